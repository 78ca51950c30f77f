// libmod16hip.so, host side: the grid handle of the downscaled families (downscale.hip creates and
// destroys it; downscale.hip and composite_downscale.hip launch with it).
#pragma once
#include "host.hpp"
#include "../mod16_downscale.hpp"

// The corner tables of both axes on the device (mod16_amd/downscale.py: corner_tables) -- or, in the
// row-affine geometry (mod16_downscale_create_rows*: corner_tables_rows), the row tables and the
// per-row (origin, scale) of the columns. The geometry picks the kernel instance at launch.
struct mod16_downscale {
    int device = 0;
    mod16_downscale_spec spec = {};
    DevMem tables;               // ri0, ri1 (int32 [R]), rw0, rw1 (double [R]), the same four for the columns;
                                 // row-affine: ri0, ri1, rw0, rw1, origin, scale (double [R])
    bool affine = false;         // true: `gr` holds the views, false: `g`
    DsGrid g = {};               // views into `tables`
    DsRowsGrid gr = {};
};

// the arguments of a launch with the handle's geometry in place (G: DsGrid or DsRowsGrid)
template <typename T, typename G> static DsArgs<T, G> ds_with_grid(const DsArgs<T>& a, const G& g) {
    DsArgs<T, G> b;
    memset(&b, 0, sizeof b);
    for (int k = 0; k < 14; ++k) b.drv[k] = a.drv[k];
    b.dense = a.dense;
    b.coarse = a.coarse;
    b.g = g;
    b.cpitch = a.cpitch;
    b.first = a.first;
    b.n = a.n;
    b.cls = a.cls;
    b.lut64 = a.lut64;
    b.tab = a.tab;
    b.out_day = a.out_day;
    b.out_night = a.out_night;
    b.status = a.status;
    return b;
}
