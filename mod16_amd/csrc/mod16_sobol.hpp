// gfx950 kernels of the Sobol sensitivity analysis (mod16_sobol_*_f64, capi/sensitivity.hip;
// mod16_amd/sensitivity.py): Saltelli samples drawn on the device, the static pixel function
// evaluated on them without the samples ever existing in HBM, and the Sobol indices with their
// bootstrap as one batched weighted Gram product. float64 only.
//
// Sobol points. Dimension k of point i (unscrambled, Joe-Kuo direction numbers, 32 bits):
//     u_k(i) = 2^-32 * XOR of kSobolV[k][b] over the set bits b of gray(i) = i ^ (i >> 1)
// -- the points of scipy.stats.qmc.Sobol(d, scramble=False, bits=32) in order, bit for bit. A value
// is lo + (hi - lo) * u, with contraction off (what numpy computes).
//
// Saltelli layout (SALib's documented one). The sequence has 2D dimensions: A = 0 .. D-1,
// B = D .. 2D-1, base sample j uses point skip + j. Its R rows, in order:
//     A_j, AB_j^(i) for i = 1..D (A with column i from B),
//     [second order: BA_j^(i) for i = 1..D (B with column i from A)], B_j
// so R = 2D + 2 (D + 2 without second order), and Y is [n][R].
//
// Indices (the whole contract). With `normalize`, Y' = (Y - mean(Y)) / std(Y) over all n R values
// (ddof 0). fA = Y'[:,0], fABi = Y'[:,1+i], fBAi = Y'[:,1+D+i], fB = Y'[:,R-1]:
//     V = var(concat(fA, fB))                                 (ddof 0)
//     S1_i = mean(fB (fABi - fA)) / V
//     ST_i = 0.5 mean((fA - fABi)^2) / V
//     S2_jk = mean(fBAj fABk - fA fB) / V - S1_j - S1_k      (j < k; the rest of S2 is NaN)
// Every sum is an entry of the weighted Gram matrix z^T diag(c) z of the per-sample vector
//     z = [1, fA - s, fB - s, fAB_1 - fA .. fAB_D - fA, fBA_1 - s .. fBA_D - s]
// (s = 0 with `normalize`, else the mean of fA and fB over the whole sample: the shift is added
// back in closed form, and keeps the sums of an unnormalised Y free of cancellation). c is 1 for
// the point estimate, and for bootstrap resample r (0-based) the multiplicity of each base sample
// among its n draws:
//     draw(seed, r, k) = mix(mix(seed) ^ ((r << 32) | k)) & (n - 1),  k = 0 .. n-1
//     mix(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb;
//             z ^= z >> 31                                    (splitmix64's finaliser, uint64)
// The Gram kernel gathers the drawn rows directly (a resample's sums are over its draws in order
// k = 0, 1, ...), so no multiplicity array exists. Sums: per block in a fixed order over its chunk of
// draws, then the chunks in order (sobol_indices_kernel); no floating-point atomics -- two calls give
// the same bits. The confidence value of an index is the standard deviation (ddof 1) of its values
// over the resamples (the caller multiplies by the normal quantile).
#pragma once
#include <stdint.h>
#include "mod16_physics.hpp"

namespace mod16 {

constexpr int kSobolBlock = 256;
constexpr int kSobolMaxD = 14;                  // 2D <= 28 of the table's 32 dimensions
constexpr int kSobolMaxZ = 3 + 2 * kSobolMaxD;  // 31 components of z
constexpr int kSobolMaxEnt = kSobolMaxZ * (kSobolMaxZ + 1) / 2;   // 496 Gram entries
constexpr int kSobolSumBlocks = 256;            // partials of the moment sums (device-independent)
constexpr int kSobolGramDraws = 64;             // draws staged in LDS per step of the Gram kernel
// rows kernel: the scaled points of the base samples one block's 256 rows touch, [jj][2D]:
// nj <= 255 / R + 2 samples with R >= D + 2, so nj * 2D < 2D * 255 / (D + 2) + 4D < 566
constexpr int kSobolPts = 576;

// BEGIN SOBOL TABLE (tools/make_sobol_table.py)
static __constant__ uint32_t kSobolV[32][32] = {
    {0x80000000u, 0x40000000u, 0x20000000u, 0x10000000u, 0x08000000u, 0x04000000u, 0x02000000u, 0x01000000u,
     0x00800000u, 0x00400000u, 0x00200000u, 0x00100000u, 0x00080000u, 0x00040000u, 0x00020000u, 0x00010000u,
     0x00008000u, 0x00004000u, 0x00002000u, 0x00001000u, 0x00000800u, 0x00000400u, 0x00000200u, 0x00000100u,
     0x00000080u, 0x00000040u, 0x00000020u, 0x00000010u, 0x00000008u, 0x00000004u, 0x00000002u, 0x00000001u},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0xf0000000u, 0x88000000u, 0xcc000000u, 0xaa000000u, 0xff000000u,
     0x80800000u, 0xc0c00000u, 0xa0a00000u, 0xf0f00000u, 0x88880000u, 0xcccc0000u, 0xaaaa0000u, 0xffff0000u,
     0x80008000u, 0xc000c000u, 0xa000a000u, 0xf000f000u, 0x88008800u, 0xcc00cc00u, 0xaa00aa00u, 0xff00ff00u,
     0x80808080u, 0xc0c0c0c0u, 0xa0a0a0a0u, 0xf0f0f0f0u, 0x88888888u, 0xccccccccu, 0xaaaaaaaau, 0xffffffffu},
    {0x80000000u, 0xc0000000u, 0x60000000u, 0x90000000u, 0xe8000000u, 0x5c000000u, 0x8e000000u, 0xc5000000u,
     0x68800000u, 0x9cc00000u, 0xee600000u, 0x55900000u, 0x80680000u, 0xc09c0000u, 0x60ee0000u, 0x90550000u,
     0xe8808000u, 0x5cc0c000u, 0x8e606000u, 0xc5909000u, 0x6868e800u, 0x9c9c5c00u, 0xeeee8e00u, 0x5555c500u,
     0x8000e880u, 0xc0005cc0u, 0x60008e60u, 0x9000c590u, 0xe8006868u, 0x5c009c9cu, 0x8e00eeeeu, 0xc5005555u},
    {0x80000000u, 0xc0000000u, 0x20000000u, 0x50000000u, 0xf8000000u, 0x74000000u, 0xa2000000u, 0x93000000u,
     0xd8800000u, 0x25400000u, 0x59e00000u, 0xe6d00000u, 0x78080000u, 0xb40c0000u, 0x82020000u, 0xc3050000u,
     0x208f8000u, 0x51474000u, 0xfbea2000u, 0x75d93000u, 0xa0858800u, 0x914e5400u, 0xdbe79e00u, 0x25db6d00u,
     0x58800080u, 0xe54000c0u, 0x79e00020u, 0xb6d00050u, 0x800800f8u, 0xc00c0074u, 0x200200a2u, 0x50050093u},
    {0x80000000u, 0x40000000u, 0x20000000u, 0xb0000000u, 0xf8000000u, 0xdc000000u, 0x7a000000u, 0x9d000000u,
     0x5a800000u, 0x2fc00000u, 0xa1600000u, 0xf0b00000u, 0xda880000u, 0x6fc40000u, 0x81620000u, 0x40bb0000u,
     0x22878000u, 0xb3c9c000u, 0xfb65a000u, 0xddb2d000u, 0x78022800u, 0x9c0b3c00u, 0x5a0fb600u, 0x2d0ddb00u,
     0xa2878080u, 0xf3c9c040u, 0xdb65a020u, 0x6db2d0b0u, 0x800228f8u, 0x400b3cdcu, 0x200fb67au, 0xb00ddb9du},
    {0x80000000u, 0x40000000u, 0x60000000u, 0x30000000u, 0xc8000000u, 0x24000000u, 0x56000000u, 0xfb000000u,
     0xe0800000u, 0x70400000u, 0xa8600000u, 0x14300000u, 0x9ec80000u, 0xdf240000u, 0xb6d60000u, 0x8bbb0000u,
     0x48008000u, 0x64004000u, 0x36006000u, 0xcb003000u, 0x2880c800u, 0x54402400u, 0xfe605600u, 0xef30fb00u,
     0x7e48e080u, 0xaf647040u, 0x1eb6a860u, 0x9f8b1430u, 0xd6c81ec8u, 0xbb249f24u, 0x80d6d6d6u, 0x40bbbbbbu},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0xd0000000u, 0x58000000u, 0x94000000u, 0x3e000000u, 0xe3000000u,
     0xbe800000u, 0x23c00000u, 0x1e200000u, 0xf3100000u, 0x46780000u, 0x67840000u, 0x78460000u, 0x84670000u,
     0xc6788000u, 0xa784c000u, 0xd846a000u, 0x5467d000u, 0x9e78d800u, 0x33845400u, 0xe6469e00u, 0xb7673300u,
     0x20f86680u, 0x104477c0u, 0xf8668020u, 0x4477c010u, 0x668020f8u, 0x77c01044u, 0x8020f866u, 0xc0104477u},
    {0x80000000u, 0x40000000u, 0xa0000000u, 0x50000000u, 0x88000000u, 0x24000000u, 0x12000000u, 0x2d000000u,
     0x76800000u, 0x9e400000u, 0x08200000u, 0x64100000u, 0xb2280000u, 0x7d140000u, 0xfea20000u, 0xba490000u,
     0x1a248000u, 0x491b4000u, 0xc4b5a000u, 0xe3739000u, 0xf6800800u, 0xde400400u, 0xa8200a00u, 0x34100500u,
     0x3a280880u, 0x59140240u, 0xeca20120u, 0x974902d0u, 0x6ca48768u, 0xd75b49e4u, 0xcc95a082u, 0x87639641u},
    {0x80000000u, 0x40000000u, 0xa0000000u, 0x50000000u, 0x28000000u, 0xd4000000u, 0x6a000000u, 0x71000000u,
     0x38800000u, 0x58400000u, 0xea200000u, 0x31100000u, 0x98a80000u, 0x08540000u, 0xc22a0000u, 0xe5250000u,
     0xf2b28000u, 0x79484000u, 0xfaa42000u, 0xbd731000u, 0x18a80800u, 0x48540400u, 0x622a0a00u, 0xb5250500u,
     0xdab28280u, 0xad484d40u, 0x90a426a0u, 0xcc731710u, 0x20280b88u, 0x10140184u, 0x880a04a2u, 0x84350611u},
    {0x80000000u, 0x40000000u, 0xe0000000u, 0xb0000000u, 0x98000000u, 0x94000000u, 0x8a000000u, 0x5b000000u,
     0x33800000u, 0xd9c00000u, 0x72200000u, 0x3f100000u, 0xc1b80000u, 0xa6ec0000u, 0x53860000u, 0x29f50000u,
     0x0a3a8000u, 0x1b2ac000u, 0xd392e000u, 0x69ff7000u, 0xea380800u, 0xab2c0400u, 0x4ba60e00u, 0xfde50b00u,
     0x60028980u, 0xf006c940u, 0x7834e8a0u, 0x241a75b0u, 0x123a8b38u, 0xcf2ac99cu, 0xb992e922u, 0x82ff78f1u},
    {0x80000000u, 0x40000000u, 0xa0000000u, 0x10000000u, 0x08000000u, 0x6c000000u, 0x9e000000u, 0x23000000u,
     0x57800000u, 0xadc00000u, 0x7fa00000u, 0x91d00000u, 0x49880000u, 0xced40000u, 0x880a0000u, 0x2c0f0000u,
     0x3e0d8000u, 0x3317c000u, 0x5fb06000u, 0xc1f8b000u, 0xe18d8800u, 0xb2d7c400u, 0x1e106a00u, 0x6328b100u,
     0xf7858880u, 0xbdc3c2c0u, 0x77ba63e0u, 0xfdf7b330u, 0xd7800df8u, 0xedc0081cu, 0xdfa0041au, 0x81d00a2du},
    {0x80000000u, 0x40000000u, 0x20000000u, 0x30000000u, 0x58000000u, 0xac000000u, 0x96000000u, 0x2b000000u,
     0xd4800000u, 0x09400000u, 0xe2a00000u, 0x52500000u, 0x4e280000u, 0xc71c0000u, 0x629e0000u, 0x12670000u,
     0x6e138000u, 0xf731c000u, 0x3a98a000u, 0xbe449000u, 0xf83b8800u, 0xdc2dc400u, 0xee06a200u, 0xb7239300u,
     0x1aa80d80u, 0x8e5c0ec0u, 0xa03e0b60u, 0x703701b0u, 0x783b88c8u, 0x9c2dca54u, 0xce06a74au, 0x87239795u},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0x50000000u, 0xf8000000u, 0x8c000000u, 0xe2000000u, 0x33000000u,
     0x0f800000u, 0x21400000u, 0x95a00000u, 0x5e700000u, 0xd8080000u, 0x1c240000u, 0xba160000u, 0xef370000u,
     0x15868000u, 0x9e6fc000u, 0x781b6000u, 0x4c349000u, 0x420e8800u, 0x630bcc00u, 0xf7ad6a00u, 0xad739500u,
     0x77800780u, 0x6d4004c0u, 0xd7a00420u, 0x3d700630u, 0x2f880f78u, 0xb1640ad4u, 0xcdb6077au, 0x824706d7u},
    {0x80000000u, 0xc0000000u, 0x60000000u, 0x90000000u, 0x38000000u, 0xc4000000u, 0x42000000u, 0xa3000000u,
     0xf1800000u, 0xaa400000u, 0xfce00000u, 0x85100000u, 0xe0080000u, 0x500c0000u, 0x58060000u, 0x54090000u,
     0x7a038000u, 0x670c4000u, 0xb3842000u, 0x094a3000u, 0x0d6f1800u, 0x2f5aa400u, 0x1ce7ce00u, 0xd5145100u,
     0xb8000080u, 0x040000c0u, 0x22000060u, 0x33000090u, 0xc9800038u, 0x6e4000c4u, 0xbee00042u, 0x261000a3u},
    {0x80000000u, 0x40000000u, 0x20000000u, 0xf0000000u, 0xa8000000u, 0x54000000u, 0x9a000000u, 0x9d000000u,
     0x1e800000u, 0x5cc00000u, 0x7d200000u, 0x8d100000u, 0x24880000u, 0x71c40000u, 0xeba20000u, 0x75df0000u,
     0x6ba28000u, 0x35d14000u, 0x4ba3a000u, 0xc5d2d000u, 0xe3a16800u, 0x91db8c00u, 0x79aef200u, 0x0cdf4100u,
     0x672a8080u, 0x50154040u, 0x1a01a020u, 0xdd0dd0f0u, 0x3e83e8a8u, 0xaccacc54u, 0xd52d529au, 0xd91d919du},
    {0x80000000u, 0xc0000000u, 0x20000000u, 0xd0000000u, 0xd8000000u, 0xc4000000u, 0x46000000u, 0x85000000u,
     0xa5800000u, 0x76c00000u, 0xada00000u, 0x6ab00000u, 0x2da80000u, 0xaabc0000u, 0x0daa0000u, 0x7ab10000u,
     0xd5a78000u, 0xbebd4000u, 0x93a3e000u, 0x3bb51000u, 0x3629b800u, 0x4d727c00u, 0x9b836200u, 0x27c4d700u,
     0xb629b880u, 0x8d727cc0u, 0xbb836220u, 0xf7c4d7d0u, 0x6e29b858u, 0x49727c04u, 0xfd836266u, 0x72c4d755u},
    {0x80000000u, 0x40000000u, 0x20000000u, 0xf0000000u, 0x38000000u, 0x14000000u, 0xf6000000u, 0x67000000u,
     0x8f800000u, 0x50400000u, 0x8aa00000u, 0x0ff00000u, 0x12a80000u, 0xabf40000u, 0xfcaa0000u, 0x28fb0000u,
     0xbd298000u, 0x0bba4000u, 0x4e06e000u, 0x330c3000u, 0x59861800u, 0xc74d3400u, 0x3d2cb200u, 0x4bb2cb00u,
     0x6e061880u, 0xc30d3440u, 0x618cb220u, 0xd342cbf0u, 0xcb2e18b8u, 0x2cb93454u, 0xe186b2d6u, 0x9349cb97u},
    {0x80000000u, 0xc0000000u, 0x20000000u, 0xf0000000u, 0x68000000u, 0x64000000u, 0x36000000u, 0x6d000000u,
     0x41800000u, 0xe0400000u, 0xd2e00000u, 0x9bf00000u, 0x0ce80000u, 0x52fc0000u, 0x5b6a0000u, 0x2fb30000u,
     0xa00c8000u, 0x30054000u, 0x4807e000u, 0x940f9000u, 0x5e01f800u, 0x090e9400u, 0x778a5600u, 0x8d416b00u,
     0x9369f880u, 0x7bb294c0u, 0xde005620u, 0xc9026bf0u, 0x578d78e8u, 0x7d4bd4a4u, 0xfb6db616u, 0x1fbefb9du},
    {0x80000000u, 0x40000000u, 0xa0000000u, 0x50000000u, 0x98000000u, 0xf4000000u, 0xae000000u, 0xbb000000u,
     0xe7800000u, 0x95c00000u, 0x1c200000u, 0xd0300000u, 0xdba80000u, 0x55f40000u, 0xff820000u, 0x21c10000u,
     0x12238000u, 0x3b3a4000u, 0xa42b6000u, 0x3430f000u, 0x4da69800u, 0x4af3ec00u, 0x2e043a00u, 0xfb0a1f00u,
     0x47851880u, 0xc5c9ac40u, 0x842f5aa0u, 0x243aef50u, 0x75a38018u, 0xeefa40b4u, 0x180b600eu, 0xb400f0ebu},
    {0x80000000u, 0xc0000000u, 0xe0000000u, 0xb0000000u, 0xb8000000u, 0x3c000000u, 0xce000000u, 0x41000000u,
     0x21800000u, 0x51c00000u, 0x09600000u, 0x85700000u, 0xf2780000u, 0x8e9c0000u, 0x60020000u, 0x70030000u,
     0x58038000u, 0x8c02c000u, 0x7602e000u, 0x7d00f000u, 0xef833800u, 0x10c10400u, 0x28e08600u, 0xd4b14700u,
     0xfb182580u, 0x0bee15c0u, 0x9279c9e0u, 0xfe9d3a70u, 0x38000008u, 0xfc00000cu, 0x2e00000eu, 0xf100000bu},
    {0x80000000u, 0xc0000000u, 0xe0000000u, 0xd0000000u, 0x68000000u, 0x3c000000u, 0x8a000000u, 0x51000000u,
     0xa9800000u, 0xddc00000u, 0x5ba00000u, 0x39d00000u, 0x95f80000u, 0x56d40000u, 0x0a020000u, 0x91030000u,
     0x49838000u, 0x0dc34000u, 0x33a1a000u, 0x05d0f000u, 0x1ffa2800u, 0x07d54400u, 0xa380a600u, 0x4cc07700u,
     0x1222ee80u, 0x3413a740u, 0xa65bf7e0u, 0x5305ab50u, 0x15f80008u, 0x96d4000cu, 0xea02000eu, 0x4103000du},
    {0x80000000u, 0x40000000u, 0x60000000u, 0xd0000000u, 0x38000000u, 0x8c000000u, 0x7e000000u, 0x71000000u,
     0xc8800000u, 0x04c00000u, 0x1ba00000u, 0xbb700000u, 0x4a980000u, 0xc3bc0000u, 0xa6020000u, 0x6d010000u,
     0xee818000u, 0x29c34000u, 0x9520e000u, 0x42b23000u, 0xe7b9f800u, 0x0d0dc400u, 0x3fb92200u, 0x110d1300u,
     0x19bbee80u, 0x3c0cadc0u, 0x973a4a60u, 0xc5cf7ef0u, 0x3a180008u, 0x0b7c0004u, 0xa3a20006u, 0x7771000du},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0x90000000u, 0x08000000u, 0x64000000u, 0x6a000000u, 0x89000000u,
     0xa5800000u, 0xcb400000u, 0x18200000u, 0xad900000u, 0xaf880000u, 0x72f40000u, 0x25820000u, 0x0b430000u,
     0xb8228000u, 0x3d924000u, 0xa7882000u, 0x16f59000u, 0x4f83a800u, 0x82412400u, 0x1da01600u, 0xf6d16d00u,
     0xbfa84080u, 0xbb672640u, 0xe0091620u, 0xf0b4efd0u, 0x38228008u, 0xfd92400cu, 0x0788200au, 0x86f59009u},
    {0x80000000u, 0xc0000000u, 0x20000000u, 0xd0000000u, 0x48000000u, 0x8c000000u, 0xd6000000u, 0x39000000u,
     0xd5800000u, 0x32400000u, 0xb2a00000u, 0x72100000u, 0x53d80000u, 0x82cc0000u, 0xcb820000u, 0x47430000u,
     0x91208000u, 0xa9534000u, 0x7cf92000u, 0x4e9e3000u, 0xfcf95800u, 0x8e9fe400u, 0xdcf9d600u, 0x5e9c8900u,
     0x94f96a80u, 0xd29fb840u, 0x42f9b760u, 0xeb9c9f30u, 0x97788008u, 0xd9df400cu, 0x25db2002u, 0xabcd300du},
    {0x80000000u, 0xc0000000u, 0x20000000u, 0x50000000u, 0xd8000000u, 0xf4000000u, 0x3e000000u, 0x95000000u,
     0x8f800000u, 0x3d400000u, 0xf3200000u, 0x2ef00000u, 0xadc80000u, 0x0a0c0000u, 0x8b220000u, 0x4af30000u,
     0x6bc88000u, 0x3b0d4000u, 0xe2a16000u, 0x16b0d000u, 0x29687800u, 0xbdbf1400u, 0x33cb5e00u, 0x0f0c2500u,
     0xfca1b480u, 0xd3b0afc0u, 0x7eeb6920u, 0x74fe4d30u, 0xfee87808u, 0xb4ff140cu, 0xdeeb5e02u, 0xe4fc2505u},
    {0x80000000u, 0x40000000u, 0xa0000000u, 0xb0000000u, 0x98000000u, 0xa4000000u, 0x7a000000u, 0xd5000000u,
     0x02800000u, 0x60400000u, 0x51e00000u, 0x88700000u, 0x8c280000u, 0x47c40000u, 0x0be20000u, 0xad710000u,
     0xb6aa8000u, 0x3386c000u, 0xb8006000u, 0x54039000u, 0x42036800u, 0xc1019400u, 0xe0826a00u, 0x11431100u,
     0x2960af80u, 0x3d3175c0u, 0xdf4a3aa0u, 0xaff49e10u, 0xd62b6808u, 0x62c59404u, 0x31606a0au, 0xd932110bu},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0x30000000u, 0x18000000u, 0x34000000u, 0x8a000000u, 0x9d000000u,
     0x67800000u, 0x82400000u, 0x40e00000u, 0x60f00000u, 0x91480000u, 0x29440000u, 0x2d620000u, 0xbfb30000u,
     0x162a8000u, 0xfbf4c000u, 0xe4ca6000u, 0xc207d000u, 0x2002a800u, 0xf001b400u, 0xb8037e00u, 0x04021900u,
     0x92034b80u, 0xa90327c0u, 0xed81f320u, 0x1f40d810u, 0x27602808u, 0xe2b1740cu, 0xd1ab1e0au, 0x49b6c903u},
    {0x80000000u, 0x40000000u, 0xe0000000u, 0xd0000000u, 0x08000000u, 0x4c000000u, 0x02000000u, 0xb5000000u,
     0x36800000u, 0xc2c00000u, 0x14200000u, 0x07500000u, 0x1bf80000u, 0x50340000u, 0x48a20000u, 0xac910000u,
     0xd35b8000u, 0xbca74000u, 0x7bfa2000u, 0xc0343000u, 0xa0a18800u, 0x30909400u, 0xd95b7a00u, 0x45a57b00u,
     0x4f7a7880u, 0xb7f6f940u, 0x82013de0u, 0xf502dfd0u, 0xd6820808u, 0x12c3d404u, 0x1c235a0eu, 0x4b504b0du},
    {0x80000000u, 0xc0000000u, 0xe0000000u, 0x50000000u, 0x68000000u, 0x4c000000u, 0x76000000u, 0xf7000000u,
     0x36800000u, 0xd7400000u, 0x87e00000u, 0xef300000u, 0xa3a80000u, 0xd5440000u, 0x23aa0000u, 0x15470000u,
     0xc3a98000u, 0x45464000u, 0xaba82000u, 0x09477000u, 0xdda9f800u, 0xfe44ac00u, 0xeb292200u, 0x2907f100u,
     0x6ccb3d80u, 0xc6344dc0u, 0xcf61b320u, 0x137318d0u, 0xeccb3d88u, 0x06344dccu, 0x2f61b32eu, 0x437318d5u},
    {0x80000000u, 0x40000000u, 0x60000000u, 0x90000000u, 0xc8000000u, 0x74000000u, 0x52000000u, 0x03000000u,
     0xeb800000u, 0x6f400000u, 0x64600000u, 0xdaf00000u, 0x17980000u, 0x297c0000u, 0xa59a0000u, 0xfa7d0000u,
     0xe61b8000u, 0x713f4000u, 0x1878a000u, 0xdcce9000u, 0xb661e800u, 0x99f29c00u, 0x9c184600u, 0xd63e2100u,
     0x09fa5780u, 0x548e0ac0u, 0xa380a9e0u, 0x5b413f30u, 0x56625788u, 0x49f20ac4u, 0x341aa9e6u, 0x323c3f39u},
    {0x80000000u, 0xc0000000u, 0xa0000000u, 0xd0000000u, 0xb8000000u, 0x04000000u, 0x6e000000u, 0x97000000u,
     0xf2800000u, 0xedc00000u, 0x13600000u, 0x5c900000u, 0xdb580000u, 0x31e40000u, 0x09da0000u, 0xcc270000u,
     0x02b88000u, 0x44b44000u, 0x0fe26000u, 0xe6505000u, 0x9ab9d800u, 0x50b50c00u, 0x79e29200u, 0xa552fb00u,
     0xbe38bf80u, 0x2e77d940u, 0xf6000ae0u, 0x830112d0u, 0x84803f88u, 0xaec3994cu, 0x37e26aeau, 0x225142ddu},
    {0x80000000u, 0xc0000000u, 0xe0000000u, 0x30000000u, 0x68000000u, 0xec000000u, 0x22000000u, 0x2b000000u,
     0x36800000u, 0x9d400000u, 0x6a200000u, 0x16700000u, 0x4de80000u, 0x330c0000u, 0x936a0000u, 0x824f0000u,
     0x3b498000u, 0x8f3fc000u, 0x28202000u, 0xcd707000u, 0xf36aa800u, 0x724fdc00u, 0xb34bf200u, 0x533e6900u,
     0x62207a80u, 0x0a7140c0u, 0xe7ea6520u, 0xc40d90f0u, 0xefe9fa88u, 0xd80e80ccu, 0x45ea452eu, 0x2f0de0f3u},
};
// END SOBOL TABLE

__device__ __forceinline__ uint32_t sobol_u32(int dim, uint64_t i) {
    uint64_t g = i ^ (i >> 1);
    uint32_t x = 0;
    for (int b = 0; g; ++b, g >>= 1)
        if (g & 1u) x ^= kSobolV[dim][b];
    return x;
}

__device__ __forceinline__ double sobol_scale(double lo, double hi, uint32_t x) {
#pragma clang fp contract(off)
    return lo + (hi - lo) * ((double)x * 0x1p-32);
}

// does column k of row `row` of a Saltelli block come from B?
__device__ __forceinline__ bool saltelli_from_b(int row, int k, int d, int R) {
    if (row == 0) return false;                  // A
    if (row == R - 1) return true;               // B
    if (row <= d) return k == row - 1;           // AB^(i)
    return k != row - 1 - d;                     // BA^(i)
}

__host__ __device__ __forceinline__ uint64_t sobol_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ int64_t sobol_draw(uint64_t seed_mixed, uint32_t r, uint32_t k, int64_t mask) {
    return (int64_t)(sobol_mix(seed_mixed ^ (((uint64_t)r << 32) | k)) & (uint64_t)mask);
}

// ---- the sample: out[n R][d], one thread per value
struct SobolSampleArgs {
    double lo[kSobolMaxD], hi[kSobolMaxD];
    int d, R;
    int64_t n;
    uint64_t skip;
    double* out;
};

__global__ void __launch_bounds__(kSobolBlock) sobol_sample_kernel(const SobolSampleArgs a) {
    const int64_t total = a.n * a.R * a.d;
    for (int64_t e = (int64_t)blockIdx.x * kSobolBlock + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * kSobolBlock) {
        const int64_t w = e / a.d;
        const int k = (int)(e - w * a.d);
        const int64_t j = w / a.R;
        const int row = (int)(w - j * a.R);
        const int dim = saltelli_from_b(row, k, a.d, a.R) ? a.d + k : k;
        a.out[e] = sobol_scale(a.lo[k], a.hi[k], sobol_u32(dim, a.skip + (uint64_t)j));
    }
}

// ---- sample, MOD16._et and output fused: Y[j][row] = day + night of that row's drivers
struct SobolRowsArgs {
    double params[11];               // MOD16.required_parameters order
    double base[14];                 // the drivers not varied
    double lo[kSobolMaxD], hi[kSobolMaxD];
    int slot[14];                    // driver -> its column among the varied ones, or -1
    int d, R;
    int64_t n;
    uint64_t skip;
    double* y;                       // [n][R]
};

__global__ void __launch_bounds__(kSobolBlock) sobol_rows_kernel(const SobolRowsArgs a) {
    __shared__ double pts[kSobolPts];
    const int64_t total = a.n * a.R;
    const int dd = 2 * a.d;
    ClassPar<double> p;
    p.tmin_close = a.params[0]; p.tmin_open = a.params[1]; p.vpd_open = a.params[2];
    p.vpd_close = a.params[3]; p.gl_sh = a.params[4]; p.gl_wv = a.params[5];
    p.g_cut = a.params[6]; p.csl = a.params[7]; p.rbl_min = a.params[8];
    p.rbl_max = a.params[9]; p.beta = a.params[10];
    for (int64_t w0 = (int64_t)blockIdx.x * kSobolBlock; w0 < total; w0 += (int64_t)gridDim.x * kSobolBlock) {
        // the block's rows touch base samples j0 .. j0 + nj - 1: their 2D scaled values, once
        const int64_t j0 = w0 / a.R;
        const int64_t wl = (w0 + kSobolBlock < total ? w0 + kSobolBlock : total) - 1;
        const int nj = (int)(wl / a.R - j0 + 1);
        __syncthreads();
        for (int e = threadIdx.x; e < nj * dd; e += kSobolBlock) {
            const int jj = e / dd, c = e - jj * dd;
            const int k = c < a.d ? c : c - a.d;
            pts[e] = sobol_scale(a.lo[k], a.hi[k], sobol_u32(c, a.skip + (uint64_t)(j0 + jj)));
        }
        __syncthreads();
        const int64_t w = w0 + threadIdx.x;
        if (w >= total) continue;
        const int64_t j = w / a.R;
        const int row = (int)(w - j * a.R);
        const double* pj = pts + (j - j0) * dd;
        auto v = [&](int k) {
            const int s = a.slot[k];
            if (s < 0) return a.base[k];
            return pj[saltelli_from_b(row, s, a.d, a.R) ? a.d + s : s];
        };
        PixelIn<double> x = {v(0), v(1), v(2), v(3), v(4), v(5), v(6), v(7), v(8), v(9), v(10), v(11), v(12), v(13)};
        bool any_gs;
        {
#pragma clang fp contract(off)
            // each row is its own MOD16._et call: the whole-array switch any(g_surf > 0) of
            // mod16/__init__.py:343-348 is this row's own
            any_gs = (gsurf_static(p, x.tmin, x.vpd_d) / rcorr_exact(x.pa, x.t_d)) > 0.0;
        }
        double day, night;
        et_static_pixel(x, p, false, 0.0, 0.0, any_gs, day, night);
        a.y[w] = day + night;
    }
}

// ---- analysis: moments (normalisation / shift), Gram partials, indices, bootstrap spread
// stats[0] = shift, stats[1] = scale, stats[2] = the shift added back (0 when normalised)
struct SobolAnalyzeArgs {
    const double* y;                 // [n][R]
    double* stats;                   // device [4]
    double* sum_partial;             // device [kSobolSumBlocks]
    double* gram;                    // device [resamples + 1][nchunks][nent]
    double* idx;                     // device [resamples + 1][nidx]
    double* out;                     // device [2][nidx]: index, spread
    int64_t n;
    int d, R, m, nent, nidx, nchunks, resamples;
    int64_t chunk;                   // draws per Gram block (a multiple of kSobolGramDraws)
    uint64_t seed_mixed;             // sobol_mix(seed)
};

template <int MODE>     // 0: sum of Y; 1: sum of the A and B columns; 2: sum of (Y - stats[0])^2
__global__ void __launch_bounds__(kSobolBlock) sobol_sum_kernel(const SobolAnalyzeArgs a) {
    __shared__ double red[kSobolBlock];
    const int64_t total = MODE == 1 ? 2 * a.n : a.n * a.R;
    const double mean = MODE == 2 ? a.stats[0] : 0.0;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kSobolBlock + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * kSobolBlock) {
#pragma clang fp contract(off)
        if (MODE == 1) {
            acc += a.y[(e >> 1) * a.R + ((e & 1) ? a.R - 1 : 0)];
        } else if (MODE == 2) {
            const double dv = a.y[e] - mean;
            acc += dv * dv;
        } else {
            acc += a.y[e];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kSobolBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.sum_partial[blockIdx.x] = red[0];
}

template <int MODE>
__global__ void __launch_bounds__(kSobolBlock) sobol_stats_kernel(const SobolAnalyzeArgs a) {
    __shared__ double red[kSobolSumBlocks];
    red[threadIdx.x] = a.sum_partial[threadIdx.x];
    __syncthreads();
    for (int s = kSobolSumBlocks / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (MODE == 0) {                 // normalise: the mean ...
        a.stats[0] = red[0] / (double)(a.n * a.R);
        a.stats[2] = 0.0;
    } else if (MODE == 1) {          // no normalisation: shift by the mean of fA and fB, scale 1
        a.stats[0] = red[0] / (double)(2 * a.n);
        a.stats[1] = 1.0;
        a.stats[2] = a.stats[0];
    } else {                         // ... and the standard deviation (ddof 0)
        a.stats[1] = __builtin_sqrt(red[0] / (double)(a.n * a.R));
    }
}

// upper-triangle entry (p <= q) of an m x m symmetric matrix, row-major
__device__ __forceinline__ int sobol_ent(int p, int q, int m) { return p * m - p * (p - 1) / 2 + (q - p); }

// block (chunk c, resample r): Gram partials of the draws k in [c chunk, (c + 1) chunk); r = 0 is the
// point estimate (draw k = sample k), r >= 1 bootstrap resample r - 1
__global__ void __launch_bounds__(kSobolBlock) sobol_gram_kernel(const SobolAnalyzeArgs a) {
    __shared__ double z[kSobolGramDraws][kSobolMaxZ + 1];
    const int r = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t k1 = (k0 + a.chunk < a.n) ? k0 + a.chunk : a.n;
    const double shift = a.stats[0], scale = a.stats[1];
    int p[2] = {0, 0}, q[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        int e = threadIdx.x + s * kSobolBlock, pp = 0;
        if (e >= a.nent) e = 0;
        while (e >= a.m - pp) { e -= a.m - pp; ++pp; }
        p[s] = pp;
        q[s] = pp + e;
    }
    double acc0 = 0.0, acc1 = 0.0;
    const int m = a.m, d = a.d, R = a.R;
    for (int64_t kt = k0; kt < k1; kt += kSobolGramDraws) {
        __syncthreads();
        for (int e = threadIdx.x; e < kSobolGramDraws * m; e += kSobolBlock) {
#pragma clang fp contract(off)
            const int dr = e / m, comp = e - dr * m;
            const int64_t k = kt + dr;
            double val = 0.0;
            if (k < k1) {
                const int64_t j = r == 0 ? k : sobol_draw(a.seed_mixed, (uint32_t)(r - 1), (uint32_t)k, a.n - 1);
                const double* row = a.y + j * R;
                auto f = [&](int col) { return (row[col] - shift) / scale; };
                if (comp == 0) val = 1.0;
                else if (comp == 1) val = f(0);
                else if (comp == 2) val = f(R - 1);
                else if (comp < 3 + d) val = f(comp - 2) - f(0);
                else val = f(comp - 2);            // BA^(i): column 1 + D + i = comp - 2
            }
            z[dr][comp] = val;
        }
        __syncthreads();
#pragma unroll 4
        for (int dr = 0; dr < kSobolGramDraws; ++dr) {
            acc0 = __builtin_fma(z[dr][p[0]], z[dr][q[0]], acc0);
            acc1 = __builtin_fma(z[dr][p[1]], z[dr][q[1]], acc1);
        }
    }
    double* out = a.gram + ((int64_t)r * a.nchunks + blockIdx.x) * a.nent;
    if (threadIdx.x < a.nent) out[threadIdx.x] = acc0;
    if (threadIdx.x + kSobolBlock < a.nent) out[threadIdx.x + kSobolBlock] = acc1;
}

// block r: the Gram matrix of resample r (chunks summed in order), then its indices
// [S1 d | ST d | S2 d*d] into idx[r]
__global__ void __launch_bounds__(kSobolBlock) sobol_indices_kernel(const SobolAnalyzeArgs a) {
#pragma clang fp contract(off)
    __shared__ double G[kSobolMaxEnt];
    __shared__ double s1[kSobolMaxD];
    const int r = blockIdx.x;
    for (int e = threadIdx.x; e < a.nent; e += kSobolBlock) {
        const double* src = a.gram + (int64_t)r * a.nchunks * a.nent + e;
        double s = 0.0;
        for (int c = 0; c < a.nchunks; ++c) s += src[(int64_t)c * a.nent];
        G[e] = s;
    }
    __syncthreads();
    const int m = a.m, d = a.d;
    const double back = a.stats[2];
    auto g = [&](int i, int j) { return i <= j ? G[sobol_ent(i, j, m)] : G[sobol_ent(j, i, m)]; };
    const double N = g(0, 0);
    const double mc = (g(0, 1) + g(0, 2)) / (2.0 * N);
    const double V = (g(1, 1) + g(2, 2)) / (2.0 * N) - mc * mc;
    double* out = a.idx + (int64_t)r * a.nidx;
    if (threadIdx.x < d) {
        const int i = threadIdx.x;
        const double v1 = ((g(2, 3 + i) + back * g(0, 3 + i)) / N) / V;
        s1[i] = v1;
        out[i] = v1;
        out[d + i] = ((0.5 * g(3 + i, 3 + i)) / N) / V;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < d * d; t += kSobolBlock) {
        const int j = t / d, k = t - j * d;
        double v = __builtin_nan("");
        if (m > 3 + d && j < k) {
            const int ba = 3 + d + j, dk = 3 + k;
            const double sum = g(ba, 1) + g(ba, dk) - g(1, 2) + back * ((g(0, ba) + g(0, dk)) - g(0, 2));
            v = ((sum / N) / V - s1[j]) - s1[k];
        }
        out[2 * d + t] = v;
    }
}

// one thread per index: the point estimate, and the standard deviation (ddof 1) over the resamples
__global__ void __launch_bounds__(kSobolBlock) sobol_conf_kernel(const SobolAnalyzeArgs a) {
    for (int i = threadIdx.x; i < a.nidx; i += kSobolBlock) {
#pragma clang fp contract(off)
        const int B = a.resamples;
        double mean = 0.0;
        for (int r = 1; r <= B; ++r) mean += a.idx[(int64_t)r * a.nidx + i];
        mean = mean / (double)B;
        double ss = 0.0;
        for (int r = 1; r <= B; ++r) {
            const double dv = a.idx[(int64_t)r * a.nidx + i] - mean;
            ss += dv * dv;
        }
        a.out[i] = a.idx[i];
        a.out[a.nidx + i] = __builtin_sqrt(ss / (double)(B - 1));
    }
}

}  // namespace mod16
