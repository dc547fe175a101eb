// finish_mw_layout.hpp - which layout of the microwave finish kernel a launch takes (continuum_kernel.hip, launch_finish_mw):
//   layer   finish_mw_kernel: one workgroup per (profile, layer, chunk of channels), lane = item / channel throughout
//   column  finish_mw_kernel_col<R, NW>: one workgroup of NW waves per (profile, block of 64 layers); set-up and coarse stage with
//           lane = layer, the rest with lane = channel, one layer after the other
// Pure host arithmetic like modm_plan.hpp (no HIP runtime call): tests/native/finish_mw_layout_check.cpp calls it without a GPU.
// DESIGN.md section 3.2.
#pragma once
#include <cstddef>
#include <cstring>

namespace monortm_dev {

enum { FINISH_MW_AUTO = 0, FINISH_MW_LAYER = 1, FINISH_MW_COLUMN = 2 };

// option "finish_mw" (monortm_hip_set_option, MONORTM_FINISH_MW): auto (or empty) | layer | column, anything else is refused
inline bool finish_mw_parse(const char *v, int *out) {
    if (!v || !*v || !strcmp(v, "auto")) *out = FINISH_MW_AUTO;
    else if (!strcmp(v, "layer")) *out = FINISH_MW_LAYER;
    else if (!strcmp(v, "column")) *out = FINISH_MW_COLUMN;
    else return false;
    return true;
}

constexpr int MW_COL_STRIDE = 65;         // doubles between two items of sC[item][layer]: 64 layers + 1, so that the lanes of stage B
                                          // (different items, one layer) fall on different banks
constexpr size_t MW_COL_LDS_MAX = 40960;  // bytes per workgroup: four workgroups per compute unit

// dynamic LDS of a column workgroup: the coarse values of 64 layers and one set of the four ABSRB grids per wave
inline size_t finish_mw_col_lds(int nA, int NPTABS, int nw) {
    return sizeof(double) * ((size_t)nA * MW_COL_STRIDE + (size_t)nw * 4 * (size_t)(NPTABS + 4));
}

struct MwLayoutIn {
    int nprof, nlay_max, nwn, cus;
    int nA, NPTABS;   // coarse items (MwSetup::off[4]) and width of the ABSRB grid of the spectral range
    bool sliced;      // partial sums of line slices are added inside the finish kernel (nslice > 1 && !slices_reduced)
    int opt;          // FINISH_MW_*
};

// waves per workgroup of the column layout, or 0: the layer layout serves the launch.
// Never column: sliced line lists (the slice sums are the work of a whole (profile, layer) workgroup) and ranges whose coarse arrays
// do not fit the LDS budget.  `column` takes it wherever it can run; `auto` where it was measured to win (LABNOTES section 30, one
// MI355X, parent and new interleaved, three repetitions): configs[3] whole (1024 profiles x 64 layers x 50 channels: 1024 workgroups
// of four waves on 256 compute units) 0.9466 - 0.9516 ms per step in the layer layout, 0.9216 - 0.9241 in the column layout.  That
// is the one shape measured in it, so the rule is drawn around it: a workgroup walks its block's layers one after the other, so the
// launch needs workgroups enough to put four waves on every SIMD - profiles x layer blocks >= 4 x compute units - blocks that are at
// least half full (>= 32 layers), and one block of channels (nwn <= 64: the per-channel values then stay in registers over the
// layers).  Smaller batches (the 128-profile shard: 128 workgroups on 256 compute units; single profiles) would leave most of the
// chip idle in this layout and keep the 64 times finer grid of the layer layout; NW = 8 / 16 were not measured.
inline int finish_mw_col_waves(const MwLayoutIn &in) {
    const int nw = 4;
    if (in.opt == FINISH_MW_LAYER || in.sliced) return 0;
    if (finish_mw_col_lds(in.nA, in.NPTABS, nw) > MW_COL_LDS_MAX) return 0;
    if (in.opt == FINISH_MW_COLUMN) return nw;
    const long long wgs = (long long)in.nprof * ((in.nlay_max + 63) / 64);
    if (in.nwn > 64 || in.nlay_max < 32 || wgs < 4ll * in.cus) return 0;
    return nw;
}

}  // namespace monortm_dev
