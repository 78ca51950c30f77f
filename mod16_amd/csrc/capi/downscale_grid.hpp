// libmod16hip.so, host side: the grid handle of the downscaled families (downscale.hip creates and
// destroys it; downscale.hip and composite_downscale.hip launch with it).
#pragma once
#include "host.hpp"
#include "../mod16_downscale.hpp"

// The corner tables of both axes on the device (mod16_amd/downscale.py: corner_tables).
struct mod16_downscale {
    int device = 0;
    mod16_downscale_spec spec = {};
    DevMem tables;               // ri0, ri1 (int32 [R]), rw0, rw1 (double [R]), the same four for the columns
    DsGrid g = {};               // views into `tables`
};
