// modm_plan.hpp - what one MODM evaluation launches, decided on the host from a dozen integers and doubles: the ABSRB grid, the tile
// of lines_kernel, whether far_kernel serves the grid and with how many levels, lines_ms_kernel and its layout, the split of a batch
// between the two line kernels, the line slices, the wave priorities, the finish kernel's variant, the LDS sizes and the grid.
// Pure arithmetic: no HIP runtime call, no context, no allocation - monortm_hip_modm_xs_dev (api.hip) fills a ModmPlanIn, calls
// modm_plan() and executes the ModmPlan; tests/native/modm_plan_check.cpp calls it without a GPU (tests/test_modm_plan_cpu.py holds
// the Python mirrors of tests/far_cases.py and tests/test_ms_prepare_passes.py to it).  DESIGN.md, "Plan, then execute".
// The measurement comments stand beside the statements they justify: they are the record of why each threshold has its value.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "device_common.hpp"

namespace monortm_dev {

// measurement switches that the plan reads (monortm_hip_set_option; a context's Opt extends this)
struct ModmPlanOpt {
    int nslice = 0;           // 0 = chosen per call
    int fair = -1;            // -1 = chosen per call, 0 / 1 wave priorities off / on
    int tile_waves = 0;       // 0 = lines_config(); 1 / 2 / 4 waves per workgroup of two-wavenumber tiles
    int far_levels = -1;      // -1 = chosen per call; 0 = lines_kernel forms the far field of dense grids itself; 1 .. 6 levels of far_kernel
    int lines_ms = -1;        // -1 = chosen per call; 0 = never lines_ms_kernel; 1 = whenever its layout fits (tests, measurements)
    int ms_items = 0;         // 0 = chosen per call; 64 / 128 / 192 (state, line) items per chunk of lines_ms_kernel
    int finish_generic = 0;   // 1 = finish_kernel also where finish_mw_kernel would serve (A/B measurements, tests of the two against each other)
};

// everything the decision reads
struct ModmPlanIn {
    // shape and caller flags
    int nprof, nwn, nlay_max, nmol, real_kind, ibrd, ixsect;
    double v1, v2;            // first / last wavenumber
    // constants of the line table
    long long nlines;
    double lines_per_cm;      // lines of the table per cm-1
    double lc_frac;           // share of the table's lines that carry line-coupling coefficients
    bool any_brd;             // the table holds species-broadening parameters
    int ms_nslot;             // (molecule, isotopologue) pairs among the first nmol molecules (lines_ms_kernel's slots)
    // constants of the device
    int cus;                  // compute units
    size_t phys_cap, far_cap; // most bytes of the line-physics records / of far_kernel's workspace
    ModmPlanOpt opt;
    bool no_physics_pass;     // MONORTM_NO_PHYSICS_PASS: A/B switch for measurements
};

// everything the execution needs
struct ModmPlan {
    double V1ABS, V2ABS;      // the ABSRB grid (modm.f90:180-185)
    int NPTABS;
    int nw, wpl;              // waves per workgroup, wavenumbers per lane of lines_kernel
    bool far_tiles;           // tiles of 128 / 256 wavenumbers chosen because far_kernel serves the grid
    int TW;                   // wavenumbers per tile
    long long ntiles;
    bool use_ms;              // lines_ms_kernel serves profiles [0, ms_nprof) (all of them unless the batch is split)
    int ms_nprof;
    MsArgs ms;                // its layout (the device pointers are the execution's)
    int nslice, fair;
    size_t partial_elems;     // line-slice workspace (0: one slice)
    bool mw;                  // finish_mw_kernel closes the call
    bool need_osum;           // ... and reads the line sums from osum
    size_t osum_elems;
    bool use_brd;             // species-broadening instantiations
    // dense grids: what the call wants (the execution falls back where a workspace cannot be had)
    bool want_phys;
    size_t phys_need;
    int far_levels;           // 0: the far field stays inside lines_kernel
    size_t far_bytes, far_mom_bytes, far_geom_bytes;
    int far_ni;
    double far_rho_tile;      // half-width of a tile (launch_far)
    size_t dyn_lds;           // lines_kernel
    unsigned grid[3];         // (tile x slice, profile, layer): see lines_kernel
    // finish kernel
    int slices_reduced;
    bool high, par, quad;
    int fin_threads, lds_sets, csize;
    size_t fin_lds;
    int finish_variant;       // 0 finish_mw_kernel, 1 finish_kernel<HIGH>, 2 <PAR>, 3 <Q4>, 4 plain with 64 threads, 5 plain with 256
};

// lines_kernel.hip: block = nw waves, lane = wpl wavenumbers (tile = wpl * nw * 64); span = wn[nwn-1] - wn[0]
inline void lines_config(int nwn, int real_kind, long long states, double span, int *nw, int *wpl) {
    if (nwn <= 64) { *nw = 1; *wpl = 1; }
    // single precision, 129 - 256 wavenumbers, a batch that fills the chip twice over even so (states = profiles x layers): ONE
    // one-wave tile with four wavenumbers per lane - the prologue and the prepare stage (double precision arithmetic in this
    // build too) are paid once per layer instead of once per tile of 128 (configs[4] whole: lines 1.398 -> 1.242 ms; its 32-
    // profile share, 4096 states, is better off with the 8192 workgroups of two tiles: 0.183 against 0.215 ms)
    // ... for channel sets that span less than half the 25 cm-1 rule (a sounder's: configs[4], 0.3 - 6.5 cm-1): there the lines'
    // classes are the same for all four wavenumbers of a lane and most two-resonance lines are FULL.  A set spread over
    // 0.3 - 30 cm-1 is better off with two tiles of half the spread each (round 3's workload: 0.843 against 0.882 ms)
    else if (real_kind == 4 && nwn > 128 && nwn <= 256 && states >= 8192 && span <= 12.5) { *nw = 1; *wpl = 4; }
    // up to 256 wavenumbers: one or two one-wave tiles of 128.  Two tiles repeat the prepare stage, but a one-wave workgroup has
    // no barrier to wait at (configs[4] whole, 200 channels: 0.860 -> 0.819 ms against one two-wave tile of 256)
    else if (nwn <= 256) { *nw = 1; *wpl = 2; }
    else { *nw = 4; *wpl = 2; }
}

// levels of far_kernel for tiles of tw wavenumbers - tiles, pairs, fours ... up to a half-width of ~3 cm-1 (configs[2], tiles of
// 0.64: three levels 1.01 ms, four 1.06, two 1.63) - and the bytes of its workspace (sums, interval geometry, candidate runs)
inline int far_levels_for(const ModmPlanIn &in, int tw) {
    if (in.nwn < 2) return 0;
    const int nt = (in.nwn + tw - 1) / tw;
    const double rho_tile = 0.5 * tw * (in.v2 - in.v1) / (double)(in.nwn - 1);
    // no interval for which a line can be far: a far line lies >= kappa half-widths from the tile's centre AND holds the whole
    // tile inside its 25 cm-1 window, i.e. kappa rho <= 25 - rho (wide sparse channel sets: the plan, the levels and the
    // workspace would be paid for nothing - ADVICE r5).  far_kernel counts the workgroups of a molecule on an XCD in 16 bits
    // (FarPlace::cnt): a grid of more tiles than that keeps the far field inside lines_kernel
    if (MONORTM_FAR_KAPPA * rho_tile >= 25.0 - rho_tile || nt > 65535) return 0;
    int levels = 1;
    while (levels < FAR_MAXLEV && rho_tile * (double)(1 << levels) <= 3.0 && far_level_count(nt, levels - 1) > 1) levels++;
    if (in.opt.far_levels >= 0) levels = std::min(in.opt.far_levels, FAR_MAXLEV);
    return levels;
}
inline size_t far_bytes_for(const ModmPlanIn &in, int tw, int levels, size_t *mom_b, size_t *geom_b) {
    const int nt = (in.nwn + tw - 1) / tw;
    const size_t ni = (size_t)far_level_offset(nt, levels), states = (size_t)in.nprof * in.nlay_max;
    *mom_b = states * ni * in.nmol * FAR_MOM_STRIDE * sizeof(double);
    *geom_b = states * ni * in.nmol * FAR_GEOM_INTS * sizeof(int);
    return *mom_b + *geom_b + states * (size_t)nt * in.nmol * FAR_SEG_INTS * sizeof(int);
}

// LDS bytes of a wave of lines_ms_kernel (lines_ms_kernel.hip: ms_lds)
inline size_t lines_ms_lds(const MsArgs &ms, int nmol) {
    return MS_HOTA_BYTES * (size_t)(ms.G * ms.sa_stride) + sizeof(double) * (size_t)(64 + ms.G * 20 + ms.G * nmol + 2 * ms.G * ms.nslot) +
           sizeof(unsigned long long) * (size_t)(4 + MS_MAXSTEPS + 2 * MS_WPS + 1) + sizeof(int) * (size_t)(3 * nmol + 2 + 64) + (size_t)ms.nsteps * 64 + 16;
}

// MONORTM_OK and *p, or MONORTM_EARG and *why
inline int modm_plan(const ModmPlanIn &in, ModmPlan *p, const char **why) {
    const int nprof = in.nprof, nwn = in.nwn, nlay_max = in.nlay_max, nmol = in.nmol;
    *p = ModmPlan{};
    const double DVABS = 1.0;
    const double V1ABS = (int)(in.v1) - 3. * DVABS;
    const double V2ABS = (int)(in.v2 + 3. * DVABS + 0.5);
    const int NPTABS = (int)((V2ABS - V1ABS) / DVABS + 1.5);
    if (NPTABS > 5050) { *why = "wavenumber span exceeds the 5050-point continuum grid (N_ABSRB, lblparams.f90:35)"; return MONORTM_EARG; }
    if (nprof > 65535) { *why = "more than 65535 profiles in one call: split the batch"; return MONORTM_EARG; }
    p->V1ABS = V1ABS; p->V2ABS = V2ABS; p->NPTABS = NPTABS;

    // few workgroups (single profiles): slice the line list over several blocks per (profile, layer, tile)
    int nw, wpl;  // waves per workgroup, wavenumbers per lane
    lines_config(nwn, in.real_kind, (long long)nprof * nlay_max, in.v2 - in.v1, &nw, &wpl);
    const long long nlines = in.nlines;
    // dense grids (a line sits in the window of many tiles): its tile-independent part once per (profile, layer) - 48 B of room (32 written for an uncoupled line) per
    // (layer, line), up to an eighth of the device memory; lines_kernel then reads the record instead of forming it in every tile
    const size_t phys_need = (size_t)nprof * nlay_max * (size_t)nlines * 48;
    // dense grids whose far field comes from far_kernel (the physics pass below: >= 4 tiles, records fit): tiles of two waves, 256
    // wavenumbers.  The lines a tile evaluates directly are those within 1.2 of ITS half-widths, so halving the tile halves that
    // work, and the level of intervals it adds to far_kernel costs less (configs[2]: lines_kernel 2.92 -> 1.84 ms, far_kernel
    // 0.71 -> 1.06 ms).  Without far_kernel the four-wave tile with its own far field stays the better one.
    const size_t kFarCap = in.far_cap;   // (beyond it lines_kernel forms the far field itself)
    bool far_tiles = false;   // tiles of 128 / 256 wavenumbers chosen because far_kernel serves the grid
    if (nw == 4 && wpl == 2 && in.opt.far_levels != 0 && !in.no_physics_pass && phys_need <= in.phys_cap) {
        // the smallest tile - one wave (128 wavenumbers), two, four - that still has ~1000 lines within 1.2 of its half-widths (the
        // ones it evaluates directly: below that the prologue of a tile outweighs them) and at least four tiles on the grid.
        // configs[2] (1800 lines per cm-1, 0.005 cm-1 steps), line-sum segment: 512 wavenumbers 3.75 ms, 256: 3.02, 128: 2.69
        const double dvm = (in.v2 - in.v1) / (double)std::max(nwn - 1, 1);
        for (int cand = 1; cand <= 2; cand *= 2) {
            const int tw = 128 * cand;
            size_t mb, gb;
            const int lv = far_levels_for(in, tw);
            if (nwn >= 4 * tw && in.lines_per_cm * 2.4 * (0.5 * tw * dvm) >= 1000. && lv > 0 && far_bytes_for(in, tw, lv, &mb, &gb) <= kFarCap) { nw = cand; far_tiles = true; break; }
        }
    }
    if (in.opt.tile_waves && wpl >= 2) { nw = in.opt.tile_waves; wpl = 2; }  // measurements only: waves per workgroup of the two-wavenumber tiles
    const int NTw = 64 * nw, TW = NTw * wpl;  // lines per chunk, wavenumbers per tile
    const long long ntiles = (nwn + TW - 1) / TW;
    const long long nblocks = ntiles * nlay_max * nprof;
    const long long cus = in.cus;  // (16 one-wave workgroups of lines_kernel are resident per compute unit: 128 VGPRs, 10 KB of LDS)
    p->nw = nw; p->wpl = wpl; p->far_tiles = far_tiles; p->TW = TW; p->ntiles = ntiles;
    // batches of states on a sparse channel set, double precision: G states per wave, five wavenumbers per lane
    // (lines_ms_kernel.hip) - when the batch makes whole rounds of such waves and the layout fits the LDS (decided before the line
    // slices: this kernel walks the whole list of its states)
    bool use_ms = false;
    int ms_nprof = nprof;   // profiles [0, ms_nprof) go through lines_ms_kernel (all of them unless the batch is split, below)
    MsArgs ms{};
    if (in.real_kind == 8 && nw == 1 && wpl == 1 && nlines > 0 && in.opt.lines_ms != 0 && in.opt.nslice == 0) {
        const int LPS = (nwn + MS_WPS - 1) / MS_WPS;
        int G = std::min(std::min(12, 64 / LPS), nprof);
        // slots of the molecules of this call: slot_base[nmol] pairs
        ms.nslot = in.ms_nslot;
        // lines per chunk: a prepare pass holds spp = 64 / CL whole states (a lane then keeps its line through the passes of a chunk),
        // so CL is one of the values that leave few lanes idle, the largest whose ceil(G / spp) passes stay within the budget - three
        // passes of 64 (state, line) items, two, or one - and that leaves <= 10 KB of LDS a wave (16 waves per compute unit)
        static const int cl_set[] = {64, 32, 21, 16, 12, 10, 9, 8};
        for (int items = in.opt.ms_items ? in.opt.ms_items : 192; items >= 64 && !use_ms && G >= 1 && ms.nslot > 0; items -= 64) {
            int CL = 0;
            for (int cand : cl_set)
                if (CL == 0 && (G + 64 / cand - 1) / (64 / cand) <= items / 64) CL = cand;
            if (CL == 0) break;
            ms.G = G; ms.LPS = LPS; ms.CL = CL; ms.spp = 64 / CL; ms.nsteps = (G + ms.spp - 1) / ms.spp;
            // records per state in LDS: the chunk + 2 read ahead, padded so that the states' arrays start 24 banks apart (a lane reads
            // 16 bytes of ITS state's record: eight states then touch eight disjoint groups of four banks)
            ms.sa_stride = CL + 2;
            while (ms.sa_stride % 8 != 3) ms.sa_stride++;
            ms.npg = (nprof + G - 1) / G;
            ms.inv_cl = (65536 + CL - 1) / CL;
            ms.inv_lps = (65536 + LPS - 1) / LPS;
            bool exact = ms.nsteps <= MS_MAXSTEPS;
            for (int ln = 0; ln < 64 && exact; ln++) exact = (int)(((unsigned)ln * (unsigned)ms.inv_lps) >> 16) == ln / LPS;
            for (int ln = 0; ln < 64 && exact; ln++) exact = (int)(((unsigned)ln * (unsigned)ms.inv_cl) >> 16) == ln / CL;
            if (exact && lines_ms_lds(ms, nmol) <= 10240 - 160) use_ms = true;
        }
        const long long groups = (long long)ms.npg * nlay_max;
        if (use_ms && in.opt.lines_ms < 0) {
            // auto: a wave of lines_ms_kernel carries G states, so a batch is a few ROUNDS of such waves over the 16 wave slots of
            // every compute unit, and a round that is only part full costs half a round + half its share (measured on configs[3]'s
            // shape, 50 channels, final kernels: 128 / 256 / 320 / 384 / 512 / 640 / 768 / 1024 profiles = 0.34 / 0.67 / 0.84 / 1.0 / 1.34 /
            // 1.68 / 2.0 / 2.67 rounds take 0.69 / 0.83 / 0.98 / 1.0 / 1.63 / 1.74 / 1.96 / 2.64 times the 0.35 ms of a full round;
            // lines_kernel takes 1.26 of that per round of states whatever the batch: tools/rounds_sweep.sh).
            // From two rounds on the part-full round hides behind the others (2.0 -> 1.96, 2.67 -> 2.65).  Lists with many coupled lines
            // (their shapes go one wavenumber at a time here, Voigt pairs through a queue per wave): bench's c2lc shape at 384 profiles
            // 0.524 against 0.551 ms - a margin of 5 % instead of 20 %, so only whole rounds and large batches take this kernel.
            const double r = (double)groups / (double)(16 * cus), fr = r - std::floor(r);
            const double cost_ms = (r >= 2.0) ? r : std::floor(r) + (fr > 0.02 ? 0.5 + 0.5 * fr : 0.0);
            // What lines_kernel costs per round of lines_ms_kernel's states: 1.26 at six states a wave (50 channels).  A wave's evaluate stage
            // and prologue cost the same for four states as for nine, its prepare stage goes with the states: per state 0.055 + 0.60 / G of
            // a six-state wave's time (stage times of DESIGN 3.1m), lines_kernel the same per state whatever the channel count
            // (tools/rounds_sweep.sh with MONORTM_BENCH_CHANNELS: 64 channels = four states a wave 1.01, 40 = eight 1.42, 32 = nine 1.33).
            // Species broadening (IBRD = 1: both kernels walk the seven-species blocks in every pass - 0.472 against 0.534 ms at 384
            // profiles of bench's c4brd shape) and coupled lists (above) narrow the margin.
            double gain = std::min(1.35, 1.26 * 0.155 / (0.055 + 0.60 / (double)G));
            if (in.lc_frac > 0.02) gain *= 1.04 / 1.26;
            else if (in.ibrd != 0 && in.any_brd) gain *= 1.13 / 1.26;
            // between one and two rounds: the whole rounds through lines_ms_kernel, the rest of the profiles through lines_kernel (two
            // launches on the stream; 512 profiles of configs[3]'s shape: 384 + 128 = 0.37 + 0.16 ms against 0.60 either way)
            const long long npg_round = (16 * cus) / std::max(nlay_max, 1);   // groups of G profiles that fill the wave slots once
            const long long n_whole = (long long)G * npg_round * (long long)std::floor(r);
            const double cost_split = (r >= 1.0 && r < 2.0 && n_whole >= G && n_whole < nprof)
                                          ? std::floor(r) + gain * (double)(((nprof - n_whole + G - 1) / G) * nlay_max) / (double)(16 * cus) : 1e30;
            if (G * nwn * 10 < 64 * MS_WPS * 7) use_ms = false;
            else if (cost_split < 0.97 * std::min(cost_ms, gain * r)) ms_nprof = (int)n_whole;
            else if (cost_ms >= gain * r) use_ms = false;
        }
        if (use_ms && ms_nprof < nprof) ms.npg = (ms_nprof + G - 1) / G;
    }
    p->use_ms = use_ms; p->ms_nprof = ms_nprof; p->ms = ms;
    int nslice = 1;
    if (nblocks < 4 * cus && nlines >= 2 * NTw) {
        // at least ~40 lines per slice: below that the prologue of a workgroup outweighs its share of the lines
        nslice = (int)std::min<long long>(16, std::min<long long>((8 * cus + nblocks - 1) / nblocks, nlines / 40));
        if (nslice < 1) nslice = 1;
    } else {
        // long line lists: a block walks hundreds of chunks, and with only a few rounds of blocks over the chip
        // (resident: 16 one-wave or 4 four-wave blocks per CU) the last round runs half empty.  Slices of >= 32 chunks
        // until there are >= 8 rounds.
        // (a grid served by far_kernel walks a quarter of its window at most: four rounds - configs[2], one-wave tiles: three
        // slices 2.33 ms for the line-sum segment, five 2.34, seven 2.36, two 2.40, one 2.64)
        const long long resident = cus * (16 / nw), chunks = nlines / NTw;
        const long long want = ((far_tiles ? 4 : 8) * resident + nblocks - 1) / nblocks;
        nslice = (int)std::max<long long>(1, std::min<long long>(16, std::min<long long>(want, chunks / 32)));
        // a grid that fills at most five eighths of the wave slots: two slices use the rest (c4 shape, 32 profiles: 0.096 ->
        // 0.089 ms per step).  A full round is better off unsliced since the waves order themselves by progress (a.fair below):
        // 64 profiles 0.155 -> 0.127 ms, c5 0.188 -> 0.151 ms per step
        if (nslice == 1 && nblocks * nw <= 10 * cus && nlines >= 3 * NTw) nslice = 2;
    }
    if (in.opt.nslice) nslice = in.opt.nslice;  // measurements only
    if (use_ms) nslice = 1;   // (lines_ms_kernel walks the whole list of its states)
    p->nslice = nslice;
    if (nslice > 1) p->partial_elems = (size_t)nslice * nprof * nlay_max * nmol * nwn;
    // progress-ordered wave priorities (lines_kernel.hip): grids of at most a few rounds over the 4096 wave slots that 128 VGPRs
    // leave on 256 CUs.  Re-measured in round 4 with the shorter kernels: one-wave double-precision tiles gain at every size
    // (4 / 8 / 16 rounds: -3 % / -0.6 % / -0.5 %), the four-wavenumber float tile loses at 8 rounds (configs[4] whole: 1.127
    // against 1.099 ms), multi-wave tiles lose 1 % at 8, the one-wave two-wavenumber tile gains 2 % at 8 (round 3's configs[4]
    // workload: 0.823 against 0.841 ms) - so: always for the first, up to 8 rounds for the last, up to 4 for the others
    // (round 5, after the tested sub-runs are skipped per (wave, k): the four-wavenumber float tile gains at 8 rounds as well -
    // configs[4] whole 0.992 -> 0.948 ms - so every one-wave tile up to 8 rounds)
    p->fair = ((nw == 1 && wpl == 1 && in.real_kind == 8) || nblocks * nslice * nw <= ((nw == 1) ? 8 : 4) * 16 * cus) ? 1 : 0;
    if (in.opt.fair >= 0) p->fair = in.opt.fair;  // measurements only
    // microwave to far infrared (last wavenumber below 820 cm-1: no O3 / O2 / Rayleigh term anywhere): the fused finish kernel
    // (option "finish" = generic: an A/B switch for measurements and tests)
    const bool mw = in.v2 < 820.0 && NPTABS <= 1000 && !in.opt.finish_generic;
    p->mw = mw;
#ifdef LINES_TIMING
    p->need_osum = mw;
#else
    p->need_osum = mw && nslice == 1;
#endif
    if (p->need_osum) p->osum_elems = (size_t)nprof * nlay_max * nwn;
    p->use_brd = in.ibrd != 0 && in.any_brd;
    p->dyn_lds = sizeof(double) * (size_t)(19 * nmol) + sizeof(int) * (size_t)(2 * nmol + 2 + 2 * FAR_SEGS * nmol);
#ifdef MONORTM_EXTRA_LDS   // occupancy experiment (tools/build_variant.sh): fewer resident workgroups per CU
    p->dyn_lds += MONORTM_EXTRA_LDS;
#endif
    p->grid[0] = (unsigned)(((nwn + TW - 1) / TW) * nslice); p->grid[1] = (unsigned)nprof; p->grid[2] = (unsigned)nlay_max;
    p->phys_need = phys_need;
    p->want_phys = ntiles >= 4 && nlines > 0 && phys_need <= in.phys_cap && !in.no_physics_pass;
    // multi-wave tiles (the ones that have a far field): the far lines of every tile through far_kernel
    p->far_levels = (p->want_phys && wpl == 2) ? far_levels_for(in, TW) : 0;
    if (p->far_levels > 0) {
        p->far_bytes = far_bytes_for(in, TW, p->far_levels, &p->far_mom_bytes, &p->far_geom_bytes);
        p->far_ni = far_level_offset((int)ntiles, p->far_levels);
    }
    p->far_rho_tile = 0.5 * TW * (in.v2 - in.v1) / (double)std::max(nwn - 1, 1);
    // finest coarse grid: 1 cm-1 (O2 A band) above 1340 cm-1, 2 cm-1 (CO2) below
    const bool high = in.v2 > 1340.0;
    const int csize = (high ? NPTABS : NPTABS / 2) + 24;
    // few workgroups (single profiles) below 1340 cm-1: the four waves of a workgroup run the passes side by side, each
    // with its own grids; a grid that fills the chip is served better by one pass after the other
    const bool par = !high && (long long)nlay_max * nprof < 16 * cus;
    const int fin_threads = par ? 256 : ((NPTABS <= 256 && nwn <= 128) ? 64 : 256);  // microwave-sized grids: one wave
    // one-wave workgroups on a grid of >= 4096 of them: four layers per wave, a 16-lane team each (continuum_kernel.hip)
    const bool quad = !high && !par && fin_threads == 64 && NPTABS <= 64;
    const int lds_sets = (par || quad) ? 4 : 1;
    p->high = high; p->par = par; p->quad = quad; p->fin_threads = fin_threads; p->lds_sets = lds_sets; p->csize = csize;
    p->fin_lds = sizeof(double) * (size_t)(NPTABS + 4 + csize) * lds_sets;
    p->slices_reduced = (nslice > 1 && (long long)nmol * nwn > 4096) ? 1 : 0;  // wide grids: the slice sums at full memory bandwidth
    p->finish_variant = mw ? 0 : (high ? 1 : (par ? 2 : (quad ? 3 : (fin_threads == 64 ? 4 : 5))));
    return MONORTM_OK;
}

}  // namespace monortm_dev
