// The launch plan of one MODM evaluation (monortm_amd/csrc/modm_plan.hpp) from the command line: one ModmPlanIn per line of stdin, the
// fields of its ModmPlan (or the refusal) on one line of stdout.  Built and driven by tests/test_modm_plan_cpu.py (no GPU: host code only).
// Input, separated by blanks (doubles in any form strtod reads, hexadecimal included):
//   nprof nwn nlay_max nmol real_kind ibrd ixsect v1 v2 nlines lines_per_cm lc_frac any_brd ms_nslot cus phys_cap far_cap
//   nslice fair tile_waves far_levels lines_ms ms_items finish_generic no_physics_pass
// Output: name=value pairs; doubles as hexadecimal floats (exact).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../monortm_amd/csrc/modm_plan.hpp"

using namespace monortm_dev;

int main() {
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n' || line[0] == '#') continue;
        ModmPlanIn in{};
        int any_brd = 0, nopp = 0;
        unsigned long long phys_cap = 0, far_cap = 0;
        const int got = std::sscanf(line, "%d %d %d %d %d %d %d %la %la %lld %la %la %d %d %d %llu %llu %d %d %d %d %d %d %d %d", &in.nprof, &in.nwn,
                                    &in.nlay_max, &in.nmol, &in.real_kind, &in.ibrd, &in.ixsect, &in.v1, &in.v2, &in.nlines, &in.lines_per_cm,
                                    &in.lc_frac, &any_brd, &in.ms_nslot, &in.cus, &phys_cap, &far_cap, &in.opt.nslice, &in.opt.fair,
                                    &in.opt.tile_waves, &in.opt.far_levels, &in.opt.lines_ms, &in.opt.ms_items, &in.opt.finish_generic, &nopp);
        if (got != 25) { std::fprintf(stderr, "modm_plan_check: %d of 25 fields in: %s", got, line); return 2; }
        in.any_brd = any_brd != 0; in.no_physics_pass = nopp != 0;
        in.phys_cap = (size_t)phys_cap; in.far_cap = (size_t)far_cap;
        ModmPlan p;
        const char *why = "";
        const int rc = modm_plan(in, &p, &why);
        if (rc) { std::printf("rc=%d why=%s\n", rc, why); continue; }
        std::printf("rc=0 V1ABS=%a V2ABS=%a NPTABS=%d nw=%d wpl=%d far_tiles=%d TW=%d ntiles=%lld use_ms=%d ms_nprof=%d G=%d LPS=%d CL=%d spp=%d nsteps=%d "
                    "sa_stride=%d npg=%d inv_cl=%d inv_lps=%d nslot=%d ms_lds=%zu nslice=%d fair=%d partial_elems=%zu mw=%d need_osum=%d osum_elems=%zu "
                    "use_brd=%d want_phys=%d phys_need=%zu far_levels=%d far_bytes=%zu far_mom_bytes=%zu far_geom_bytes=%zu far_ni=%d far_rho_tile=%a "
                    "dyn_lds=%zu grid_x=%u grid_y=%u grid_z=%u slices_reduced=%d high=%d par=%d quad=%d fin_threads=%d lds_sets=%d csize=%d fin_lds=%zu "
                    "finish_variant=%d\n",
                    p.V1ABS, p.V2ABS, p.NPTABS, p.nw, p.wpl, (int)p.far_tiles, p.TW, p.ntiles, (int)p.use_ms, p.ms_nprof, p.ms.G, p.ms.LPS, p.ms.CL,
                    p.ms.spp, p.ms.nsteps, p.ms.sa_stride, p.ms.npg, p.ms.inv_cl, p.ms.inv_lps, p.ms.nslot, p.use_ms ? lines_ms_lds(p.ms, in.nmol) : (size_t)0,
                    p.nslice, p.fair, p.partial_elems, (int)p.mw, (int)p.need_osum, p.osum_elems, (int)p.use_brd, (int)p.want_phys, p.phys_need,
                    p.far_levels, p.far_bytes, p.far_mom_bytes, p.far_geom_bytes, p.far_ni, p.far_rho_tile, p.dyn_lds, p.grid[0], p.grid[1], p.grid[2],
                    p.slices_reduced, (int)p.high, (int)p.par, (int)p.quad, p.fin_threads, p.lds_sets, p.csize, p.fin_lds, p.finish_variant);
    }
    return 0;
}
