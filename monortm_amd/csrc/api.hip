// api.hip - host side of the C ABI (include/monortm_hip.h): context, TAPE3 -> device line table, model tables,
// launch configuration, host-buffer front ends for the Fortran shim.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "line_table.hpp"
#include "modm_plan.hpp"
#include "finish_mw_layout.hpp"
#include "lineshape.hpp"
#include "tables/monortm_tables.h"

namespace {
using namespace monortm_dev;

// ------------------------------------------------------------------------------------------------
// host side: context, uploads, launches
// ------------------------------------------------------------------------------------------------
thread_local std::string g_init_error;

struct Ctx {
    int device = 0;
    int cus = 256;            // compute units of the device (MI355X: 256): the launch heuristics count wave slots with it
    // workspaces of dense grids may grow to a share of the device's memory (MI355X: 288 GB -> 36 GB of line-physics records, 9 GB of
    // far-field sums; a grid that needs more has its line physics formed in place and its far field inside lines_kernel)
    size_t phys_cap = 2ull << 30, far_cap = 1ull << 30;
    // multi-device context (monortm_hip_init_multi): no device resources of its own, one full context per device
    std::vector<Ctx *> shards;
    // measurement switches (monortm_hip_set_option; the environment variables MONORTM_NSLICE / _FAIR /
    // _TILE_WAVES / _FINISH_GENERIC give their defaults ONCE, when the context is created - nothing on the launch path calls getenv)
    struct Opt : ModmPlanOpt {   // (modm_plan.hpp: the switches that decide what a MODM evaluation launches)
        int ms_ablate = 0;        // timing experiments: lines_ms_kernel without its later stages (wrong results)
        int ms_prepare = MS_PREPARE_FUSED;   // lines_ms_kernel's prepare stage: the fused trip where it applies / the pass loop always
        int ms_plan = 1;          // lines_ms_kernel: the launch-wide chunk plan for the waves that match it / every wave on its own
        int finish_mw = monortm_dev::FINISH_MW_AUTO;   // layout of the microwave finish kernel (finish_mw_layout.hpp)
        double jac_dt = MONORTM_JAC_DT, jac_dlnw = MONORTM_JAC_DLNW;   // half-steps of the Jacobian's central differences
    } opt;
    void *comm = nullptr;     // RCCL communicator of a multi-process job (monortm_hip_comm_init), one rank per context
    int comm_rank = 0, comm_world = 1;
    bool has_lines = false;  // a TAPE3 was loaded (a context created with an empty path serves RTM / CALCTMR only)
    int real_kind = 8;  // element size of the caller's REAL arrays (the reference's "dbl" / "sgl" builds)
    std::string err;
    monortm::LineTable host;
    DevLines lines{};
    DevTables tables{};
    std::vector<void *> owned;
    int *errflag = nullptr;
    void *partial = nullptr;  // line-slice workspace, grown on demand
    monortm_dev::MwCache mw_cache;  // spectral-range constants of finish_mw_kernel (launch_finish_mw)
    void *phys = nullptr;     // per (profile, layer, line) LinePhys records of dense grids (physics_kernel), grown on demand
    size_t phys_bytes = 0;
    void *far = nullptr;      // far_kernel's sums, interval geometry and candidate runs of dense grids, grown on demand
    size_t far_bytes = 0;
    double lines_per_cm = 0.;           // lines of the table per cm-1 (the tile choice of dense grids, far_kernel's workgroups); 0: no lines
    bool no_physics_pass = false;       // MONORTM_NO_PHYSICS_PASS (A/B switch for measurements), read once per process when the first context is created
    hipStream_t far_stream = nullptr;   // far_plan_kernel runs beside physics_kernel (fork / join with far_ev)
    hipEvent_t far_ev[2] = {nullptr, nullptr};
    // lines_ms_kernel (batches of states on sparse channel sets): slot of (molecule, isotopologue 1) among the isotopologues the
    // table holds - on the device and here - and the scratch of the rare shapes, grown on demand
    double lc_frac = 0.;      // share of the table's lines that carry line-coupling coefficients
    const int *ms_slot_base = nullptr;
    int ms_slot_host[MXMOL + 1] = {0};
    void *ms_scratch = nullptr;
    unsigned short *ms_reach = nullptr;  // per table line: the slots of channels it / its negative resonance can reach (ms_reach_kernel)
    size_t ms_scratch_bytes = 0;
    void *ms_plan = nullptr;  // the chunk plan of lines_ms_kernel (device_common.hpp, MS_PLAN_*): rewritten by every launch, grown on demand
    size_t ms_plan_words = 0;
    double *osum = nullptr;   // per (profile, layer, wn) line sums handed from lines_kernel to finish_mw_kernel, grown on demand
    size_t osum_elems = 0;
    DevXsec xs{};             // cross-section tables (monortm_hip_xsec_tables); xs_buf holds them, replaced as a whole
    std::vector<void *> xs_buf;
    // staging arenas of the host-buffer entry points (HostCall), grown on demand and kept: a caller that loops over profiles (the
    // reference's driver does) pays for device allocations once, not per call.  Twelve slots = three groups of four (pinned host
    // input arena, device input arena, pinned host output arena, device output arena; even slots are the pinned ones): 0-3 MODM, 4-7
    // RTM and the path scans, 8-11 every Jacobian entry - so that lastO, which points into slots 2 and 3, stays valid across a
    // Jacobian call made between a MODM and an RTM call
    struct Stage {
        void *p = nullptr;
        size_t bytes = 0;
    };
    Stage stage[12];
    // monortm_hip_jacobian_dev: the MODM inputs and optical depths of the base and the perturbed states, and the outputs of MODM
    // that the Jacobian does not use, grown on demand and kept (a second call of the same shapes allocates nothing)
    void *jac_ws = nullptr;
    size_t jac_ws_bytes = 0;
    // monortm_hip_oe_step_dev: the workspace [nprof][2][nmeas][nstate] of oe_kernel.hip, and the state map on
    // the device with the host copy it was uploaded from - a call whose map equals the copy uploads nothing.  Grown on demand and kept
    void *oe_ws = nullptr;
    size_t oe_ws_elems = 0;
    void *oe_map = nullptr;
    size_t oe_map_ints = 0;
    std::vector<int> oe_map_host;
    // monortm_hip_oe_step_full_dev asked for dofs without avk_diag: the diagonal that the kernel sums, [nprof][nstate]
    void *oe_diag = nullptr;
    size_t oe_diag_elems = 0;
    // monortm_hip_oe_scatter_dev (section 3.15): the write map on the device and the host copy it was uploaded from, kept like the state map
    void *oe_wmap = nullptr;
    size_t oe_wmap_ints = 0;
    std::vector<int> oe_wmap_host;
    // measurement operators (monortm_hip_obs_create): the device tables of up to kMaxObs operators, checked on
    // the host when they were created - the kernel never sees an unchecked index, and a call that takes a handle copies nothing
    struct Obs {
        int handle = 0;   // 0 = free
        int npath = 0, nwn = 0, nview = 0, nchan = 0;
        void *dev = nullptr;   // one allocation: wpath, mw, view_start, mstart, mlane
        const int *view_start = nullptr, *mstart = nullptr, *mlane = nullptr;
        const double *wpath = nullptr, *mw = nullptr;
        std::vector<int> shard;   // multi-device context: the operator's handle on every shard
    };
    static constexpr int kMaxObs = 16;
    Obs obs[kMaxObs];
    // The host-buffer entry points run on their own stream: one asynchronous upload, the kernels, one asynchronous
    // download (+ the 4-byte error flag) and a single synchronisation per call.
    hipStream_t hs = nullptr;
    int *errflag_host = nullptr;  // pinned
    // What the last host-buffer MODM left behind: the total optical depths O on the device and their pinned host copy.
    // The reference's driver hands exactly these values to CALCTMR and RTM next (monortm.f90:557-574); when the caller's
    // O compares equal to the copy, monortm_hip_rtm reads the resident array instead of uploading it again.
    struct {
        const void *dev = nullptr, *host = nullptr;
        size_t bytes = 0;
        int nprof = 0, nwn = 0, nlay_max = 0;
    } lastO;
    long long o_reused = 0;  // calls of monortm_hip_rtm that found O resident
    long long o_reused_scan = 0;  // calls of monortm_hip_rtm_scan that did
    // launches of the continuum / cloud / total kernel by variant (monortm_hip_counter 2 .. 7): finish_mw_kernel, finish_kernel<HIGH>,
    // <PAR>, <Q4>, plain with 64 threads, plain with 256
    long long finish_launches[6] = {0, 0, 0, 0, 0, 0};
    // ... of which finish_mw_kernel_col, the column layout of variant 0 (monortm_hip_counter 9)
    long long finish_mw_col_launches = 0;
    // launches of far_kernel by waves per workgroup (monortm_hip_counter 16 .. 19): 1, 2, 4, 8 - one per level and MODM evaluation
    long long far_launches[4] = {0, 0, 0, 0};
    // MONORTM_HOST_TIMING=1: wall time of the host-buffer calls by phase (pack, enqueue, wait, unpack), printed at finalize
    bool host_timing = false;
    double ht[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // modm, rtm, rtm_scan
    long long ht_calls[3] = {0, 0, 0};
    size_t partial_elems = 0;
    int profiling = 0;  // bit k set: record events around kernel k
    int prof_stride = 1;  // ... around every prof_stride-th launch of it (an event pair costs a few microseconds of the stream)
    long long prof_calls[3] = {0, 0, 0};
    struct Ev {
        hipEvent_t a, b;
        int k;
    };
    std::vector<Ev> events;
    std::vector<hipEvent_t> event_pool;  // events are created once and reused: no hipEventCreate inside a timed region
    double tot_ms[3] = {0, 0, 0};
    long long launches[3] = {0, 0, 0};
};

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return MONORTM_EHIP;                                                                     \
        }                                                                                            \
    } while (0)

// Small host-buffer calls (one profile per call - the reference driver's pattern) move their arenas with a copy KERNEL
// that reads / writes the pinned host arena directly over PCIe: a DMA-engine copy costs tens of microseconds of latency
// each, a few hundred KB through a kernel a few.  Large batches keep hipMemcpyAsync.
constexpr size_t kKernelCopyMax = 4u << 20;
__global__ __launch_bounds__(256) void copy16_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16,
                                                     const uint4 *__restrict__ src2, uint4 *__restrict__ dst2, size_t n16b,
                                                     const int *flag_src, int *flag_dst) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x == gridDim.x - 1)
        for (size_t i = threadIdx.x; i < n16b; i += 256) dst2[i] = src2[i];
    if (flag_dst && blockIdx.x == 0 && threadIdx.x == 0) *flag_dst = *flag_src;  // error flags of the kernels before this one
}
// arenas and their pieces are multiples of 256 bytes (Arena::add); the optional second piece (src2 -> dst2) is small
hipError_t move_arena(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s, const int *flag_src = nullptr,
                      int *flag_dst = nullptr, void *dst2 = nullptr, const void *src2 = nullptr, size_t bytes2 = 0) {
    if (bytes <= kKernelCopyMax) {
        const size_t n16 = bytes / 16;
        const unsigned blocks = (unsigned)std::min<size_t>(256, std::max<size_t>(1, (n16 + 255) / 256));
        hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const uint4 *>(src), static_cast<uint4 *>(dst), n16,
                           static_cast<const uint4 *>(src2), static_cast<uint4 *>(dst2), bytes2 / 16, flag_src, flag_dst);
        return hipGetLastError();
    }
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
    if (e == hipSuccess && flag_dst) e = hipMemcpyAsync(flag_dst, flag_src, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && bytes2) e = hipMemcpyAsync(dst2, src2, bytes2, hipMemcpyDefault, s);
    return e;
}

void comm_release(Ctx *c);  // (RCCL communicator of the context, defined with the gather entry points)

// one measurement switch from its textual value; unknown names / values are refused (MONORTM_EARG)
int set_option(Ctx *c, const char *name, const char *value) {
    const std::string n = name ? name : "", v = value ? value : "";
    const bool autov = v.empty() || v == "auto";
    long iv = 0;
    int iopt = 0;
    double dv = 0.;
    bool isint = false, isdbl = false;
    if (!autov) {
        char *end = nullptr;
        iv = strtol(v.c_str(), &end, 10);
        isint = end && end != v.c_str() && *end == '\0';
        end = nullptr;
        dv = strtod(v.c_str(), &end);
        isdbl = end && end != v.c_str() && *end == '\0';
    }
    if (n == "nslice" && (autov || (isint && iv >= 1 && iv <= 16))) c->opt.nslice = autov ? 0 : (int)iv;
    else if (n == "fair" && (autov || (isint && (iv == 0 || iv == 1)))) c->opt.fair = autov ? -1 : (int)iv;
    else if (n == "tile_waves" && (autov || (isint && (iv == 1 || iv == 2 || iv == 4)))) c->opt.tile_waves = autov ? 0 : (int)iv;
    else if (n == "far_levels" && (autov || (isint && iv >= 0 && iv <= FAR_MAXLEV))) c->opt.far_levels = autov ? -1 : (int)iv;
    // lines_kernel: auto = by batch size; wn = lines_kernel (one state per wave) always; ms = lines_ms_kernel (several states per wave,
    // five wavenumbers per lane) wherever its layout fits (double precision, <= 64 wavenumbers)
    else if (n == "lines_kernel" && (autov || v == "wn" || v == "ms")) c->opt.lines_ms = autov ? -1 : (v == "ms" ? 1 : 0);
    // ms_prepare: auto = fused = a plain chunk of two or three prepare passes in one trip per lane (lines_ms_kernel.hip, ms_prepare_trip);
    // passes = the pass loop for every chunk (A/B measurements, tests of the two against each other: identical bits)
    else if (n == "ms_prepare" && (autov || v == "fused" || v == "passes")) c->opt.ms_prepare = v == "passes" ? MS_PREPARE_PASSES : MS_PREPARE_FUSED;
    // ms_plan: auto = on = a wave whose states all match the launch-wide chunk plan (lines_ms_kernel.hip, ms_plan_wave) copies its windows
    // and the words of its plain chunks from it; off = every wave searches and ballots for itself (A/B measurements, tests: identical bits)
    else if (n == "ms_plan" && (autov || v == "on" || v == "off")) c->opt.ms_plan = v == "off" ? 0 : 1;
#ifdef MONORTM_EXPERIMENT   // stage ablations of lines_ms_kernel: timing only, wrong results - experiment builds alone know the option
    else if (n == "ms_ablate" && isint && iv >= 0 && iv <= 9) c->opt.ms_ablate = (int)iv;
#endif
    // continuum / cloud / total kernel: auto = finish_mw_kernel below 820 cm-1, finish_kernel elsewhere; generic = finish_kernel always
    else if (n == "finish" && (autov || v == "generic")) c->opt.finish_generic = autov ? 0 : 1;
    // finish_mw_kernel's layout: auto = by batch size (finish_mw_col_waves); layer = a workgroup per (profile, layer) always; column = a
    // workgroup per (profile, block of 64 layers) wherever that layout can run (A/B measurements, tests of the two: identical bits)
    else if (n == "finish_mw" && monortm_dev::finish_mw_parse(v.c_str(), &iopt)) c->opt.finish_mw = iopt;
    else if (n == "ms_items" && (autov || (isint && (iv == 64 || iv == 128 || iv == 192 || iv == 256)))) c->opt.ms_items = autov ? 0 : (int)iv;
    // half-steps of the Jacobian: a finite positive double (jac_dlnw below 1: WKL (1 - eps) stays positive)
    else if ((n == "jac_dt" || n == "jac_dlnw") && (autov || (isdbl && std::isfinite(dv) && dv > 0. && (n == "jac_dt" || dv < 1.)))) {
        if (n == "jac_dt") c->opt.jac_dt = autov ? MONORTM_JAC_DT : dv;
        else c->opt.jac_dlnw = autov ? MONORTM_JAC_DLNW : dv;
    }
    else { c->err = "unknown option or value: " + n + " = " + v; return MONORTM_EARG; }
    return MONORTM_OK;
}

template <class T>
int upload(Ctx *c, const T *src, size_t n, const T **dst) {
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(c, hipMalloc(&p, bytes));
    c->owned.push_back(p);
    if (n) HIPCHK(c, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(p);
    return MONORTM_OK;
}

void prof_begin(Ctx *c, hipStream_t s, int k, Ctx::Ev &ev) {
    ev.k = -1;
    if (!((c->profiling >> k) & 1)) return;
    if (c->prof_stride > 1 && (c->prof_calls[k]++ % c->prof_stride) != 0) return;
    auto take = [&](hipEvent_t *e) {
        if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); }
        else hipEventCreate(e);
    };
    take(&ev.a);
    take(&ev.b);
    ev.k = k;
    hipEventRecord(ev.a, s);
}
void prof_end(Ctx *c, hipStream_t s, Ctx::Ev &ev) {
    if (ev.k < 0) return;
    hipEventRecord(ev.b, s);
    c->events.push_back(ev);
}

// A workspace grown on demand: at least `need` elements of `elem` bytes behind *p, *have of them there now.  Growth frees the old block
// first (the contents are not kept); on failure the workspace is empty and the error is returned - the caller fails or falls back.
hipError_t grow(void **p, size_t *have, size_t need, size_t elem = 1) {
    if (need <= *have) return hipSuccess;
    hipError_t e = *p ? hipFree(*p) : hipSuccess;
    *p = nullptr;
    *have = 0;
    if (e == hipSuccess) e = hipMalloc(p, need * elem);
    if (e == hipSuccess) *have = need;
    else *p = nullptr;
    return e;
}

// Ctx::jac_ws with room for `bytes`: the workspace of the Jacobian entries and of monortm_hip_obs_dev - whichever call needs more grows it
int jac_ws_reserve(Ctx *c, size_t bytes) {
    HIPCHK(c, grow(&c->jac_ws, &c->jac_ws_bytes, bytes));
    return MONORTM_OK;
}

// the *_dev entry points launch on the calling thread's current device: it must be the context's
int check_device(Ctx *c) {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d != c->device) {
        c->err = "the context was created on device " + std::to_string(c->device) + " but device " + std::to_string(d) +
                 " is current: call hipSetDevice (torch.cuda.set_device) before the *_dev entry points";
        return MONORTM_EARG;
    }
    return MONORTM_OK;
}

int check_modm_args(Ctx *c, int nprof, int nwn, int nlay_max, int nmol, int ibrd, int ixsect, double v2) {
    if (nprof < 1 || nwn < 1 || nlay_max < 1 || nlay_max > 603) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (nmol < 7 || nmol > MXMOL) { c->err = "nmol must be 7..39 (LINES reads WK(1:7), modm.f90:313)"; return MONORTM_EARG; }
    if (nwn > 80000) { c->err = "nwn exceeds NWNMX=80000 (RTMmono.f90:10)"; return MONORTM_EARG; }
    if (ixsect != 0 && ixsect != 1) { c->err = "ixsect must be 0 or 1"; return MONORTM_EARG; }
    if (ibrd != 0 && !c->host.any_brd) { /* nothing to do: flags all zero, same as ibrd = 0 */ }
    (void)v2;
    return MONORTM_OK;
}

// Dense grids, ahead of lines_kernel: physics_kernel's records and far_kernel's sums where the plan wants them and their workspaces
// can be had (a.phys / a.farmom stay null otherwise: lines_kernel forms the records, or the far field, itself)
int dense_passes(Ctx *c, const ModmPlan &pl, ModmArgs &a, hipStream_t s) {
    const int nlines = (int)c->host.size();
    // (a workspace a later call needs less than a quarter of - or not at all - goes back to the device: a single large dense call
    // must not pin tens of GB away from the caller's framework for the life of the context)
    if (c->phys && (!pl.want_phys || pl.phys_need < c->phys_bytes / 4) && c->phys_bytes > (64u << 20)) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cap);
        if (cap == hipStreamCaptureStatusNone) {
            HIPCHK(c, hipDeviceSynchronize());   // (nobody reads the records any more)
            HIPCHK(c, hipFree(c->phys));
            c->phys = nullptr;
            c->phys_bytes = 0;
            if (c->far) { HIPCHK(c, hipFree(c->far)); c->far = nullptr; c->far_bytes = 0; }
        }
    }
    if (pl.want_phys) {
        // no room for the records: lines_kernel forms them in place, as on sparse grids
        if (grow(&c->phys, &c->phys_bytes, pl.phys_need) != hipSuccess) (void)hipGetLastError();
        if (c->phys) {
            a.phys = c->phys;
            a.phys_lines = nlines;
            if (pl.far_levels > 0) {
                if (pl.far_bytes > c->far_bytes && pl.far_bytes <= c->far_cap) {   // (beyond the cap lines_kernel forms the far field itself)
                    if (grow(&c->far, &c->far_bytes, pl.far_bytes) == hipSuccess) {
                        // all-ones bytes = NaN sums, -1 indices: an entry that a kernel reads without another having written it
                        // shows in the results at once instead of depending on what the allocation held (once per growth)
                        HIPCHK(c, hipMemsetAsync(c->far, 0xFF, pl.far_bytes, s));
                    } else (void)hipGetLastError();   // no room: lines_kernel forms the far field itself
                }
                if (c->far && pl.far_bytes <= c->far_bytes) {
                    a.farmom = static_cast<double *>(c->far);
                    a.fargeom = reinterpret_cast<int *>(static_cast<char *>(c->far) + pl.far_mom_bytes);
                    a.farseg = reinterpret_cast<int *>(static_cast<char *>(c->far) + pl.far_mom_bytes + pl.far_geom_bytes);
                    a.far_levels = pl.far_levels;
                    a.far_ni = pl.far_ni;
                    a.far_tw = pl.TW;
                    a.far_ntile = (int)pl.ntiles;
                }
            }
            // far_plan_kernel (a chain of dependent table reads, ~65 us whatever the grid) needs nothing physics_kernel writes: it
            // runs beside it on a stream of the context, forked from and joined to the caller's stream with two events (the pattern a
            // stream capture follows as well)
            const bool far_on = a.farmom != nullptr;
            if (far_on && !c->far_stream) {
                if (hipStreamCreateWithFlags(&c->far_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->far_ev[0], hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&c->far_ev[1], hipEventDisableTiming) != hipSuccess) {
                    c->err = "stream / events of the far-field plan could not be created";
                    return MONORTM_EHIP;
                }
            }
            if (far_on) {
                HIPCHK(c, hipEventRecord(c->far_ev[0], s));
                HIPCHK(c, hipStreamWaitEvent(c->far_stream, c->far_ev[0], 0));
                launch_far_plan(a, c->lines, c->tables, c->far_stream);
                HIPCHK(c, hipEventRecord(c->far_ev[1], c->far_stream));
            }
            launch_physics(a, c->lines, c->tables, nlines, pl.use_brd, s);
            if (far_on) {
                HIPCHK(c, hipStreamWaitEvent(s, c->far_ev[1], 0));
                launch_far(a, c->lines, c->tables, pl.far_rho_tile, c->lines_per_cm > 0. ? c->lines_per_cm : 1., c->far_launches, s);
            }
        }
    }
    return MONORTM_OK;
}

Ctx *g_timing_ctx = nullptr;
void print_host_timing(Ctx *c) {
    if (!c->host_timing) return;
    static const char *const names[3] = {"modm", "rtm ", "scan"};
    for (int k = 0; k < 3; k++)
        if (c->ht_calls[k])
            fprintf(stderr, "monortm_hip %s: %lld calls, us per call: pack %.1f enqueue %.1f wait %.1f unpack %.1f\n", names[k],
                    c->ht_calls[k], c->ht[k][0] / c->ht_calls[k] * 1e6, c->ht[k][1] / c->ht_calls[k] * 1e6,
                    c->ht[k][2] / c->ht_calls[k] * 1e6, c->ht[k][3] / c->ht_calls[k] * 1e6);
}

// device pointers, streams and kernel timers belong to ONE device: a multi-device context serves the host-buffer calls
int multi_only_host(Ctx *c) {
    c->err = "multi-device context: only monortm_hip_modm / monortm_hip_rtm (host buffers) shard over devices; create one "
             "context per device with monortm_hip_init for the *_dev / profiling entry points";
    return MONORTM_EARG;
}

int null_ctx() {
    g_init_error = "null context";
    return MONORTM_EARG;
}

// The host-buffer entry points and the multi-device set-up switch devices (hipSetDevice is per thread): the caller's current
// device is put back on every return path, so that allocations and *_dev calls made afterwards land where they did before.
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() { if (hipGetDevice(&saved) != hipSuccess) saved = -1; }
    ~DeviceGuard() { if (saved >= 0) (void)hipSetDevice(saved); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

}  // namespace

// ---- host-buffer front ends (what the Fortran shim calls): stage through device memory -----------
// All inputs of a call are packed into one pinned host arena and travel in ONE host-to-device copy, all outputs come back
// in ONE device-to-host copy: a caller that loops over profiles (the reference's driver does) pays two synchronous
// copies per call instead of one per argument.  The arenas grow on demand and stay with the context.
namespace {
struct Arena {  // layout helper: 256-byte aligned pieces of one buffer
    size_t size = 0;
    size_t add(size_t bytes) {
        const size_t off = size;
        size = (size + std::max<size_t>(bytes, 8) + 255) & ~size_t(255);
        return off;
    }
};
// ---- the argument groups of a call, named ONCE -----------------------------------------------------------------------------------
// Every extern "C" entry fills these from its parameters at its top; below that line nothing takes the groups as loose parameters.
// A field an entry has no argument for stays zero / null.
struct AtmIn {   // the atmosphere: what MODM reads (an entry that is handed O fills nprof, nwn, wn, nlay, nlay_max and T only)
    int nprof = 0, nwn = 0;
    const double *wn = nullptr;
    double dvset = 0.;
    const int *nlay = nullptr;
    int nlay_max = 0, nmol = 0;
    const void *P = nullptr, *T = nullptr, *CLW = nullptr, *WKL = nullptr, *WBRODL = nullptr;
    const double *cntnm_fac = nullptr;
    double sclcpl = 0., sclhw = 0., y0res = 0.;
    int ibrd = 0, ixsect = 0;
    const void *XAMNT = nullptr;
    const double *wn_ends = nullptr;   // on the host: wn[0], wn[nwn - 1]; null: fetched from the device (one synchronisation)
};
struct SfcIn {   // the surface and what RTM is asked for
    const int *irt = nullptr;
    const void *TZ = nullptr, *tmpsfc = nullptr, *emiss = nullptr, *reflc = nullptr;
    int quantity = 0;
};
struct ScanIn {   // the paths of a scan (npath = 0, path null: the entry has none)
    int npath = 0;
    const void *path = nullptr;
    int sfc_per_path = 0;
};
struct JacReq {   // the Jacobian variables of a full Jacobian call
    int njac = 0;
    const int *jac_mol = nullptr;
};
struct JacOut {   // the outputs of the Jacobian families: O of the full entries, RAD / TB or Y, and the K arrays the family has
    void *O = nullptr, *RAD = nullptr, *TB = nullptr, *Y = nullptr;
    void *K_T = nullptr, *K_TZ = nullptr, *K_W = nullptr, *K_CLW = nullptr, *K_O = nullptr, *K_PATH = nullptr, *K_SFC = nullptr;
};
bool any_null(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!p) return true;
    return false;
}

struct HostClock {  // phase timer of a host-buffer call (only when MONORTM_HOST_TIMING=1, and for the entries that have a row of Ctx::ht)
    Ctx *c = nullptr;
    int k = -1;
    std::chrono::steady_clock::time_point t;
    void start(Ctx *c_, int k_) {
        if (k_ < 0 || !c_->host_timing) return;
        c = c_; k = k_;
        t = std::chrono::steady_clock::now();
        c->ht_calls[k]++;
    }
    void mark(int phase) {
        if (!c) return;
        const auto n = std::chrono::steady_clock::now();
        c->ht[k][phase] += std::chrono::duration<double>(n - t).count();
        t = n;
    }
};
hipError_t stage_get(Ctx *c, int slot, size_t bytes, bool pinned_host, void **out) {
    Ctx::Stage &st = c->stage[slot];
    if (st.bytes < bytes) {
        if (st.p) {
            if (pinned_host) hipHostFree(st.p);
            else hipFree(st.p);
        }
        st.p = nullptr;
        st.bytes = 0;
        const size_t want = bytes + bytes / 4;  // some head room: profiles of a run differ little in size
        const hipError_t e = pinned_host ? hipHostMalloc(&st.p, want, hipHostMallocDefault) : hipMalloc(&st.p, want);
        if (e != hipSuccess) return e;
        st.bytes = want;
    }
    *out = st.p;
    return hipSuccess;
}
}  // namespace

namespace {
int decode_flag(Ctx *c, int flag, hipStream_t s) {
    if (!flag) return MONORTM_OK;
    HIPCHK(c, hipMemsetAsync(c->errflag, 0, sizeof(int), s));
    if (flag & ERRBIT_ARG) { c->err = "device arguments: nlay[p] outside 1..nlay_max, wavenumbers not ascending or not the grid dvset promises, or a negative / non-finite path factor (monortm_hip_rtm_scan_dev, monortm_hip_rtm_scan_jac_dev, monortm_hip_scan_jacobian_dev), or a vcen that is not finite and > 0 (monortm_hip_rtm_obs_dev, monortm_hip_obs_dev)"; return MONORTM_EARG; }
    if (flag & ERRBIT_TEMP) { c->err = "TIPS: layer temperature outside 70-3000 K / partition sum <= 0 (reference STOP, tips_2003.f90:277)"; return MONORTM_ETEMP; }
    c->err = "SDVOIGT: REAL(v) < 0 (reference STOP, modm.f90:1062)";
    return MONORTM_ESDV;
}
}  // namespace

namespace {
// ---- path scans: what the scan entries check on host arguments
constexpr int kScanMaxPaths = 16384;   // 4096 path tiles: inside the grid's z range
int scan_check_args(Ctx *c, const AtmIn &atm, const ScanIn &scan) {
    if (atm.nprof < 1 || atm.nwn < 1 || atm.nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (atm.nlay_max > 603) { c->err = "nlay_max exceeds MXLAY=603 (the bound of monortm_hip_modm, which O comes from)"; return MONORTM_EARG; }
    if (scan.npath < 1 || scan.npath > kScanMaxPaths) { c->err = "npath outside 1.." + std::to_string(kScanMaxPaths); return MONORTM_EARG; }
    if (scan.sfc_per_path != 0 && scan.sfc_per_path != 1) { c->err = "sfc_per_path must be 0 or 1"; return MONORTM_EARG; }
    return MONORTM_OK;
}
template <typename R>
bool scan_path_ok(const void *path, int nprof, int npath, const int *nlay, int nlay_max, int *bp, int *bj, int *bl) {
    const R *f = static_cast<const R *>(path);
    for (int p = 0; p < nprof; p++)
        for (int j = 0; j < npath; j++)
            for (int l = 0; l < nlay[p]; l++) {
                const double v = (double)f[((size_t)p * npath + j) * nlay_max + l];
                if (!(v >= 0. && std::isfinite(v))) { *bp = p; *bj = j; *bl = l; return false; }
            }
    return true;
}

// nlay and the factors of the active layers of a whole host call: checked before anything is staged or launched, on every device
int scan_check_path(Ctx *c, const AtmIn &atm, const ScanIn &scan) {
    for (int p = 0; p < atm.nprof; p++)
        if (atm.nlay[p] < 1 || atm.nlay[p] > atm.nlay_max) { c->err = "nlay[p] outside 1..nlay_max"; return MONORTM_EARG; }
    int bp = 0, bj = 0, bl = 0;
    const bool ok = c->real_kind == 4 ? scan_path_ok<float>(scan.path, atm.nprof, scan.npath, atm.nlay, atm.nlay_max, &bp, &bj, &bl)
                                      : scan_path_ok<double>(scan.path, atm.nprof, scan.npath, atm.nlay, atm.nlay_max, &bp, &bj, &bl);
    if (!ok) {
        c->err = "path factor negative or not finite: profile " + std::to_string(bp) + " path " + std::to_string(bj) + " layer " + std::to_string(bl);
        return MONORTM_EARG;
    }
    return MONORTM_OK;
}

// ---- the Jacobian entries: what they check on host arguments
int check_quantity(Ctx *c, int quantity) {
    if (quantity != 0 && quantity != 1) { c->err = "quantity must be 0 (RAD) or 1 (TB)"; return MONORTM_EARG; }
    return MONORTM_OK;
}
// the full Jacobians difference optical depths: double arrays only (entry: the public name the message gives)
int need_real8(Ctx *c, const char *entry) {
    if (c->real_kind == 8) return MONORTM_OK;
    c->err = std::string(entry) + " needs a real_kind = 8 context (its differences of optical depths need double arrays)";
    return MONORTM_EUNSUPPORTED;
}
int jac_check_args(Ctx *c, const AtmIn &atm, int quantity) {
    if (atm.nprof < 1 || atm.nwn < 1 || atm.nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (int rcq = check_quantity(c, quantity)) return rcq;
    for (int p = 0; p < atm.nprof; p++)
        if (atm.nlay[p] < 1 || atm.nlay[p] > atm.nlay_max) { c->err = "nlay[p] outside 1..nlay_max"; return MONORTM_EARG; }
    return MONORTM_OK;
}
// Jacobian variables: the scalar arguments of MODM among the MONORTM_JVAR_* codes, and the per-layer ones
bool jac_var_scalar(int v) {
    return (v >= MONORTM_JVAR_CNTNM0 && v < MONORTM_JVAR_CNTNM0 + 7) || v == MONORTM_JVAR_SCLCPL || v == MONORTM_JVAR_SCLHW || v == MONORTM_JVAR_Y0RES;
}
bool jac_var_layer(int v, int nmol) { return (v >= 1 && v <= nmol) || v == MONORTM_JVAR_P || v == MONORTM_JVAR_WBROD; }
constexpr int kMaxXs = 38;   // MX_XS: molecules of a cross-section request (monortm_hip_xsec_tables)
bool jac_var_xs(int v) { return v >= MONORTM_JVAR_XS0 && v < MONORTM_JVAR_XS0 + kMaxXs; }
// cross-section molecules of the context's tables (every shard of a multi-device context holds the same tables)
int ctx_nxs(const Ctx *c) { return (c->shards.empty() ? c : c->shards[0])->xs.nxs; }
// ixsect, XAMNT: the two arguments of the *_xs entries (the entries without them pass 0, nullptr: a cross-section code is refused)
int jac_check_mol(Ctx *c, const AtmIn &atm, const JacReq &jq, const void *K_W) {
    const int nmol = atm.nmol, njac = jq.njac, ixsect = atm.ixsect, *jac_mol = jq.jac_mol;
    if (njac < 0 || njac > MXMOL || (njac > 0 && (!jac_mol || !K_W))) { c->err = "njac outside 0..39, or jac_mol / K_W missing"; return MONORTM_EARG; }
    if (ixsect != 0 && ixsect != 1) { c->err = "ixsect must be 0 or 1"; return MONORTM_EARG; }
    const int nxs = ctx_nxs(c);
    for (int i = 0; i < njac; i++) {
        if (jac_var_xs(jac_mol[i])) {
            if (ixsect == 0) {
                c->err = "jac_mol[" + std::to_string(i) + "] is a cross-section molecule (MONORTM_JVAR_XS0 + x): that needs ixsect = 1 (the *_xs entries)";
                return MONORTM_EARG;
            }
            if (jac_mol[i] - MONORTM_JVAR_XS0 >= nxs) {
                c->err = "jac_mol[" + std::to_string(i) + "]: cross-section molecule " + std::to_string(jac_mol[i] - MONORTM_JVAR_XS0) +
                         " is not among the " + std::to_string(nxs) + " of this context's tables";
                return MONORTM_EARG;
            }
        } else if (!jac_var_layer(jac_mol[i], nmol) && !jac_var_scalar(jac_mol[i])) {
            c->err = "jac_mol[" + std::to_string(i) + "] neither a molecule 1..nmol nor a MONORTM_JVAR_* code";
            return MONORTM_EARG;
        }
        for (int j = 0; j < i; j++)
            if (jac_mol[j] == jac_mol[i]) { c->err = "jac_mol lists variable " + std::to_string(jac_mol[i]) + " twice"; return MONORTM_EARG; }
    }
    if (ixsect == 1 && (nxs < 1 || !atm.XAMNT)) {
        c->err = "ixsect = 1: no cross-section tables on this context (monortm_hip_xsec_tables), or XAMNT missing";
        return MONORTM_EARG;
    }
    return MONORTM_OK;
}

// what the MODM passes of a full Jacobian call refuse, on host arrays: wavenumbers that do not ascend, and T +- jac_dt outside the TIPS
// range (the MODM kernels would flag the latter as well)
int check_ascending(Ctx *c, const AtmIn &atm) {
    for (int i = 1; i < atm.nwn; i++)
        if (!(atm.wn[i] >= atm.wn[i - 1])) { c->err = "wavenumbers must be ascending (the reference takes v1 = wn(1), v2 = wn(nwn), modm.f90:180-181)"; return MONORTM_EARG; }
    return MONORTM_OK;
}
int jac_check_states(Ctx *c, const AtmIn &atm) {
    if (int rc = check_ascending(c, atm)) return rc;
    const double h = c->opt.jac_dt, *Tp = static_cast<const double *>(atm.T);
    for (int p = 0; p < atm.nprof; p++)
        for (int k = 0; k < atm.nlay[p]; k++) {
            const double t = Tp[(size_t)p * atm.nlay_max + k];
            if (!(t - h >= 70. && t + h <= 3000.)) {
                c->err = "layer temperature +- jac_dt outside 70-3000 K (TIPS, tips_2003.f90:277): profile " + std::to_string(p) + " layer " + std::to_string(k);
                return MONORTM_ETEMP;
            }
        }
    return MONORTM_OK;
}

struct ModmOut {   // the outputs of a MODM evaluation ([nprof][nlay_max](x nmol / NCONT)[nwn]; ODXSEC with ixsect = 1 only)
    void *ODXSEC = nullptr, *O = nullptr, *O_BY_MOL = nullptr, *OC = nullptr, *O_CLW = nullptr;
};
int modm_dev_impl(Ctx *c, const AtmIn &atm, bool odx_given, const ModmOut &out, hipStream_t s);   // (defined with monortm_hip_modm_xs_dev, below)

// The MODM part of a Jacobian call (monortm_hip_jacobian_dev, monortm_hip_scan_jacobian_dev): jac_perturb_kernel, then MODM of the base
// and the 2 (1 + njac) perturbed states.  Small batches (single-profile retrievals underfill the GPU) go through ONE extended MODM launch
// of all states; larger ones through one launch of nprof profiles per state, of the shapes of a plain MODM call - so that alternating
// Jacobian and plain calls never resizes the MODM workspaces (an extended launch is only taken while its line-physics records stay below
// the 64 MB under which MODM keeps them).  O gets the base state; *xO_out: the states' optical depths in the context's workspace (state k
// at xO + k st, k >= 1), *st_out: elements of one state.
// ixsect = 1: the base state runs with the cross sections, as monortm_hip_modm_xs_dev does; the states T +- h and
// P (1 +- eps) take their ODXSEC from xsec_jac_kernel - the base state's walk evaluated at the perturbed (P, T), not a walk of their
// own - and the states of a cross-section molecule are written by that kernel ("+") and cleared ("-").  With ixsect = 0 every size,
// launch and result is what it was.
static int jac_states(Ctx *c, const AtmIn &atm, const JacReq &jq, void *O, hipStream_t s, double **xO_out, size_t *st_out) {
    const int nprof = atm.nprof, nwn = atm.nwn, nlay_max = atm.nlay_max, nmol = atm.nmol, njac = jq.njac, *jac_mol = jq.jac_mol;
    double vends[2];
    if (atm.wn_ends) { vends[0] = atm.wn_ends[0]; vends[1] = atm.wn_ends[1]; }
    else {   // once here, not in every MODM call below
        HIPCHK(c, hipMemcpyAsync(&vends[0], atm.wn, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&vends[1], atm.wn + nwn - 1, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    AtmIn base = atm;   // the caller's state with the grid's ends on the host: what every MODM launch below starts from
    base.wn_ends = vends;
    // Per-layer variables (molecules, P, WBRODL) are states of the perturbed arrays, in slot order; the two states of a scalar variable
    // are MODM launches of the caller's own arrays with that argument changed.  State k of O, k = 3 + 2i / 4 + 2i
    // for jac_mol[i] of either kind; the perturbed arrays hold the nps states of the base, T +- h and the per-layer variables only.
    // XRAYL is the exception among the scalars: its states are launches on ONE more state of the perturbed arrays, which holds the
    // inputs of the Rayleigh term alone (modm_scalar below).  npa: the states of the arrays; without XRAYL npa = nps, and every size
    // and launch is what it was.
    // A cross-section molecule (MONORTM_JVAR_XS0 + x) has no state of the perturbed arrays and no MODM launch at all: O is linear in
    // XAMNT, and its two states of O are the molecule's own term and zero (xsec_jac_kernel).
    const bool xs = atm.ixsect == 1;
    int lvar[MXMOL], nlv = 0, p_state = 0;   // p_state: the "+" state of MONORTM_JVAR_P in the perturbed arrays, or 0
    bool rayl = false;
    XsecJacArgs xa{};
    for (int i = 0; i < njac; i++) {
        if (jac_var_xs(jac_mol[i])) { xa.kplus[jac_mol[i] - MONORTM_JVAR_XS0] = 3 + 2 * i; continue; }
        if (!jac_var_scalar(jac_mol[i])) {
            if (jac_mol[i] == MONORTM_JVAR_P) p_state = 3 + 2 * nlv;
            lvar[nlv++] = jac_mol[i];
        }
        rayl = rayl || jac_mol[i] == MONORTM_JVAR_CNTNM0 + 6;
    }
    const int nstate = 3 + 2 * njac, nps = 3 + 2 * nlv, npa = nps + (rayl ? 1 : 0);
    const size_t npl = (size_t)nprof * nlay_max, st = npl * nwn;
    const bool ext = (long long)nps * nprof <= 64 && (size_t)nps * npl * c->host.size() * 48 <= (64u << 20);
    const size_t nj = ext ? nps : 1;   // states whose unused MODM outputs are held at once
    // ODXSEC of the states (ixsect = 1).  An extended launch reads one slot per state of the perturbed arrays, in their order (zero for the
    // states that run without the cross sections); per-state launches need the base, T +- h and P (1 +- eps) only: slots 0, 1, 2, 3, 4
    const int nodx = !xs ? 0 : ext ? nps : (p_state ? 5 : 3);
    auto odx_slot = [&](int ps) { return ext ? ps : ps <= 2 ? ps : ps == p_state ? 3 : ps == p_state + 1 ? 4 : -1; };
    Arena ws;
    const size_t w_P = ws.add(npa * npl * 8), w_T = ws.add(npa * npl * 8), w_C = ws.add(npa * npl * 8), w_B = ws.add(npa * npl * 8),
                 w_W = ws.add(npa * npl * nmol * 8), w_nl = ws.add(npa * (size_t)nprof * sizeof(int)), w_O = ws.add(nstate * st * 8),
                 w_OM = ws.add(nj * st * nmol * 8), w_OC = ws.add(nj * st * MONORTM_NCONT * 8), w_OL = ws.add(nj * st * 8),
                 w_X = xs ? ws.add(nodx * st * 8) : 0;
    if (int rc = jac_ws_reserve(c, ws.size)) return rc;
    char *wb = static_cast<char *>(c->jac_ws);
    double *xO = reinterpret_cast<double *>(wb + w_O), *xX = xs ? reinterpret_cast<double *>(wb + w_X) : nullptr;
    *xO_out = xO;
    *st_out = st;
    JacPerturbArgs pa{};
    pa.nstate = npa; pa.rayl_state = rayl ? nps : 0; pa.nprof = nprof; pa.nlay_max = nlay_max; pa.nmol = nmol; pa.dt = c->opt.jac_dt; pa.dlnw = c->opt.jac_dlnw;
    for (int i = 0; i < nlv; i++) pa.jac_mol[i] = lvar[i];
    pa.P = static_cast<const double *>(atm.P); pa.T = static_cast<const double *>(atm.T); pa.CLW = static_cast<const double *>(atm.CLW);
    pa.WKL = static_cast<const double *>(atm.WKL); pa.WBRODL = static_cast<const double *>(atm.WBRODL); pa.nlay = atm.nlay;
    pa.xP = reinterpret_cast<double *>(wb + w_P); pa.xT = reinterpret_cast<double *>(wb + w_T); pa.xCLW = reinterpret_cast<double *>(wb + w_C);
    pa.xWBRODL = reinterpret_cast<double *>(wb + w_B); pa.xWKL = reinterpret_cast<double *>(wb + w_W); pa.xnlay = reinterpret_cast<int *>(wb + w_nl);
    launch_jac_perturb(pa, s);
    HIPCHK(c, hipGetLastError());
    if (xs) {
        // the further states' ODXSEC and the named molecules' terms, in one pass over the base state's walk; the perturbed (P, T) are
        // read from the perturbed arrays, so they are the very values the states' MODM launches see
        xa.nprof = nprof; xa.nwn = nwn; xa.nlay_max = nlay_max; xa.nx = p_state ? 4 : 2;
        xa.wn = atm.wn; xa.P = pa.P; xa.T = pa.T; xa.XAMNT = static_cast<const double *>(atm.XAMNT); xa.nlay = atm.nlay;
        xa.xP = pa.xP; xa.xT = pa.xT;
        const int pst[4] = {1, 2, p_state, p_state + 1};
        for (int i = 0; i < xa.nx; i++) { xa.pstate[i] = pst[i]; xa.oslot[i] = odx_slot(pst[i]); }
        xa.ODX = xX; xa.xO = xO; xa.stride = st; xa.two_eps = 2. * c->opt.jac_dlnw;
        if (ext && nps > 3) HIPCHK(c, hipMemsetAsync(xX + 3 * st, 0, (size_t)(nps - 3) * st * 8, s));   // (the P slots are written below)
        launch_xsec_jac(xa, c->xs, s);
        HIPCHK(c, hipGetLastError());
        if (ext) {   // the base state's ODXSEC, by xsec_kernel on the caller's arrays: what monortm_hip_modm_xs_dev launches
            ModmArgs ma{};
            ma.real_kind = 8; ma.nprof = nprof; ma.nwn = nwn; ma.nlay_max = nlay_max; ma.wn = atm.wn; ma.P = atm.P; ma.T = atm.T; ma.nlay = atm.nlay;
            ma.XAMNT = atm.XAMNT; ma.ODXSEC = xX; ma.nxs = c->xs.nxs;
            launch_xsec(ma, c->xs, s);
            HIPCHK(c, hipGetLastError());
        }
    }
    // MODM of n profiles of the perturbed arrays from their state s0 on.  States of molecules and WBRODL run WITHOUT the cross sections
    // (ODXSEC does not depend on WKL or WBRODL and would cancel in their differences): ixsect = 0 in a launch of their own, a zero slot
    // of ODXSEC inside an extended launch.  (The MODM outputs that the Jacobian does not use go to the workspace.)
    auto outputs = [&](void *Oout, void *odx) { return ModmOut{.ODXSEC = odx, .O = Oout, .O_BY_MOL = wb + w_OM, .OC = wb + w_OC, .O_CLW = wb + w_OL}; };
    auto perturbed = [&](AtmIn m, int s0) {   // m with the layer arrays of the perturbed arrays' state s0 (nlay: set by the caller)
        const size_t l0 = (size_t)s0 * npl;
        m.P = pa.xP + l0; m.T = pa.xT + l0; m.CLW = pa.xCLW + l0; m.WKL = pa.xWKL + l0 * nmol; m.WBRODL = pa.xWBRODL + l0;
        m.ixsect = 0; m.XAMNT = nullptr;
        return m;
    };
    auto modm = [&](int n, int s0, void *Oout) {
        const int slot = xs ? odx_slot(s0) : -1;
        AtmIn m = perturbed(base, s0);
        m.nprof = n; m.nlay = pa.xnlay + (size_t)s0 * nprof; m.ixsect = slot >= 0 ? 1 : 0;
        return modm_dev_impl(c, m, slot >= 0, outputs(Oout, slot >= 0 ? xX + (size_t)slot * st : nullptr), s);
    };
    // state k of O for a scalar variable: the caller's arrays, the argument at +eps (odd k) / -eps.  MODM switches a continuum off at a
    // factor <= 0, so where fac - eps <= 0 the pair is fac + 2 eps / fac: one-sided over the same 2 eps, exact for a linear factor.
    // (ixsect = 0 whatever the call's: ODXSEC depends on none of the scalars and would cancel in the difference.)
    auto modm_scalar = [&](int k, void *Oout) -> int {
        const int v = jac_mol[(k - 3) >> 1];
        const bool plus = !((k - 3) & 1);
        const double e = c->opt.jac_dlnw;
        double fac[7];
        if (jac_var_xs(v)) {   // "+": xsec_jac_kernel has written it; "-": zero
            if (!plus) HIPCHK(c, hipMemsetAsync(Oout, 0, st * 8, s));
            return MONORTM_OK;
        }
        if (v == MONORTM_JVAR_CNTNM0 + 6) {
            // XRAYL.  Rayleigh has no slot of OC - it is added into O directly - and is 1e-11 .. 1e-10 of O in the infrared: +-eps of it
            // in the total is quantisation (what XCO2C was below 30 cm-1).  Its states hold the term itself instead: MODM on the
            // state of the perturbed arrays that leaves nothing but Rayleigh (WKL = 0: no line, no other continuum; CLW = 0; WBRODL
            // = WTOT, all the term reads besides T), the other six factors 0, XRAYL = 2 eps against XRAYL = 0 - and at 0 MODM
            // switches the term off, so that state IS zero and is cleared, not launched.  O+ - O- = 2 eps dO/dXRAYL on the term's
            // own scale, exact at any XRAYL >= 0 (O is linear in it; at 0 the derivative from the positive side); below 820 cm-1
            // both states are exactly 0.
            if (!plus) { HIPCHK(c, hipMemsetAsync(Oout, 0, st * 8, s)); return MONORTM_OK; }
            for (int i = 0; i < 7; i++) fac[i] = 0.;
            fac[6] = 2. * e;
            AtmIn m = perturbed(base, nps);
            m.cntnm_fac = fac;
            return modm_dev_impl(c, m, false, outputs(Oout, nullptr), s);
        }
        AtmIn m = base;
        m.ixsect = 0; m.XAMNT = nullptr;
        for (int i = 0; i < 7; i++) fac[i] = atm.cntnm_fac[i];
        if (v >= MONORTM_JVAR_CNTNM0 && v < MONORTM_JVAR_CNTNM0 + 7) {
            double &f = fac[v - MONORTM_JVAR_CNTNM0];
            if (f - e <= 0.) f += plus ? 2. * e : 0.;
            else f += plus ? e : -e;
            m.cntnm_fac = fac;
        } else
            (v == MONORTM_JVAR_SCLCPL ? m.sclcpl : v == MONORTM_JVAR_SCLHW ? m.sclhw : m.y0res) += plus ? e : -e;
        if (int rc = modm_dev_impl(c, m, false, outputs(Oout, nullptr), s)) return rc;
        // A continuum factor reaches O through ONE addend, its molecule's slot of OC (O = lines + sum of OC + cloud, continuum_kernel.hip),
        // and the adjoints read a state only in the difference O+ - O-.  The state therefore holds that slot instead of the total: a
        // continuum of 1e-12 of O (CO2 in the microwave) would vanish in the total's rounding, its slot keeps 16 digits of its own.
        // (XRAYL: above.)
        static const int oc_slot[7] = {0, 0, 1, 2, 3, 4, -1};   // XSELF, XFRGN: H2O; XCO2C; XO3CN; XO2CN; XN2CN: slots of molecules 1, 2, 3, 7, 22
        const int slot = (v >= MONORTM_JVAR_CNTNM0 && v < MONORTM_JVAR_CNTNM0 + 7) ? oc_slot[v - MONORTM_JVAR_CNTNM0] : -1;
        if (slot >= 0)
            HIPCHK(c, hipMemcpy2DAsync(Oout, (size_t)nwn * 8, wb + w_OC + (size_t)slot * nwn * 8, (size_t)MONORTM_NCONT * nwn * 8, (size_t)nwn * 8,
                                       npl, hipMemcpyDeviceToDevice, s));
        return MONORTM_OK;
    };
    // (a cross-section molecule's states are no MODM launch either: they interrupt a run of per-layer states as a scalar's do)
    auto scalar_state = [&](int k) { return k >= 3 && (jac_var_scalar(jac_mol[(k - 3) >> 1]) || jac_var_xs(jac_mol[(k - 3) >> 1])); };
    int k = 0, ps = 0;   // the next state of O, and of the perturbed arrays
    if (!ext) {
        // the base state straight from the caller's arrays, into the caller's O: what monortm_hip_modm_dev (ixsect = 1: _modm_xs_dev, its
        // ODXSEC into slot 0) returns for them
        if (int rc = modm_dev_impl(c, base, false, outputs(O, xX), s)) return rc;
        k = ps = 1;
    }
    while (k < nstate) {
        if (scalar_state(k)) {
            if (int rc = modm_scalar(k, xO + k * st)) return rc;
            k++;
            continue;
        }
        int n = 1;   // ext: the run of per-layer states up to the next scalar variable in ONE launch (all of them when none is named)
        while (ext && k + n < nstate && !scalar_state(k + n)) n++;
        if (int rc = modm(n * nprof, ps, xO + k * st)) return rc;
        k += n;
        ps += n;
    }
    if (ext) HIPCHK(c, hipMemcpyAsync(O, xO, st * 8, hipMemcpyDeviceToDevice, s));
    return MONORTM_OK;
}

// What the full-Jacobian *_dev entries (monortm_hip_jacobian_dev, _scan_jacobian_dev, _obs_jacobian_dev) refuse first, and the chain
// fields their adjoint launches share: the perturbed states' optical depths (jac_states) and the half-steps of the differences.
int jac_full_check(Ctx *c, const char *entry, bool null, const AtmIn &atm, int quantity, const JacReq &jq, const void *K_W) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (int rc = need_real8(c, entry)) return rc;
    if (null) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rc = check_quantity(c, quantity)) return rc;
    if (atm.nmol < 7 || atm.nmol > MXMOL) { c->err = "nmol must be 7..39 (LINES reads WK(1:7), modm.f90:313)"; return MONORTM_EARG; }
    if (int rc = jac_check_mol(c, atm, jq, K_W)) return rc;
    if (atm.nprof < 1 || atm.nprof > 65535 || atm.nwn < 1 || atm.nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    return MONORTM_OK;
}
// the fields all Rtm*Args share (O: the optical depths the launch reads), and those of the scans among them
template <class Args>
void rtm_args(Args &a, const AtmIn &atm, const SfcIn &sfc, const void *O) {
    a.nprof = atm.nprof; a.nwn = atm.nwn; a.nlay_max = atm.nlay_max;
    a.wn = atm.wn; a.T = atm.T; a.TZ = sfc.TZ; a.O = O; a.emiss = sfc.emiss; a.reflc = sfc.reflc; a.nlay = atm.nlay; a.irt = sfc.irt;
}
template <class Args>
void scan_args(Args &a, const ScanIn &scan) {
    a.npath = scan.npath; a.path = scan.path; a.sfc_per_path = scan.sfc_per_path;
}
// ... and what the adjoints (RtmJacArgs, RtmScanJacArgs, RtmObsJacArgs) take besides: the quantity, TMPSFC as an input, the K arrays of all three
template <class Args>
void adjoint_args(Args &a, const AtmIn &atm, const SfcIn &sfc, const void *O, const JacOut &out) {
    rtm_args(a, atm, sfc, O);
    a.quantity = sfc.quantity; a.tmpsfc = sfc.tmpsfc;
    a.K_T = out.K_T; a.K_TZ = out.K_TZ; a.K_SFC = out.K_SFC;
}
template <class Args>   // RtmJacArgs, RtmScanJacArgs, RtmObsJacArgs
void jac_chain_args(Args &a, const Ctx *c, int njac, void *K_W, void *K_CLW, const double *xO, size_t st) {
    a.real_kind = 8; a.njac = njac; a.K_W = K_W; a.K_CLW = K_CLW;
    a.Opert = xO + st;
    a.state_stride = st;
    a.dt = c->opt.jac_dt;
    a.dlnw = c->opt.jac_dlnw;
}

// ---- sharding of a host-buffer call over the devices of a multi-device context (monortm_hip_init_multi) ------------
// Profiles are independent (src/monortm.f90:357 is a loop without cross-iteration data flow): device g takes the
// contiguous block [g ceil(P/G), (g+1) ceil(P/G)) of the batch, every device holds the whole line table, each block
// comes back over its own device's PCIe link straight into the caller's arrays.
void shard_block(int nprof, int G, int g, int *p0, int *n) {
    const int per = (nprof + G - 1) / G;
    *p0 = std::min(nprof, g * per);
    *n = std::min(nprof, *p0 + per) - *p0;
}

// double -> the context's REAL kind, rounded once (real_kind = 4), or a plain copy
void obs_unpack(void *dst, const char *src, size_t n, int real_kind) {
    if (real_kind == 8) { memcpy(dst, src, n * 8); return; }
    const double *s = reinterpret_cast<const double *>(src);
    float *d = static_cast<float *>(dst);
    for (size_t i = 0; i < n; i++) d[i] = (float)s[i];
}

// ---- the arrays of a host-buffer call, declared ONCE ----------------------------------------------------
// Every public host-buffer entry lists its array arguments here - host pointer, bytes per profile, direction - and run() does the
// rest from that one list: it lays the pieces of one device's share out in the two arenas, packs ptr + p0 stride for n stride bytes,
// uploads once, hands the entry's launch lambda the device address of every declared array, downloads once and, when the stream has
// drained, unpacks to ptr + p0 stride.  A multi-device context runs one share per shard (shard_block), enqueues on every device before
// it waits for the first, and reports the first error as "device N: ...".  A null pointer declares an absent array (the optional
// outputs; the entries' own checks have refused a null anywhere else): no piece, and the launch lambda gets null for it.
struct HostCall {
    static constexpr int kMaxFields = 24;
    enum Dir { IN, OUT, INOUT };
    struct Field {
        const void *in = nullptr;   // the caller's array: read (IN, INOUT) ...
        void *out = nullptr;        // ... and written (OUT, INOUT)
        size_t stride = 0;          // bytes per profile on the device; of a shared array: all of it
        Dir dir = IN;
        bool shared = false;        // the same for every profile (wn): never shifted, uploaded whole to every device
        bool zeroed = false;        // output cleared on the device and NOT copied back (TB of an RTM call with iout /= 1)
        bool widened = false;       // output held as double on the device, rounded once to the context's REAL kind when unpacked
    };
    // one share in flight: what finish() needs once everything is enqueued
    struct Pending {
        Ctx *s = nullptr;
        int p0 = 0, n = 0;
        char *hout = nullptr, *dout = nullptr;
        size_t off[kMaxFields] = {0};   // the fields' pieces of the output arena
        HostClock hc;
    };
    using PreFn = int (*)(const void *, Ctx *, int, int);
    using LaunchFn = int (*)(const void *, Ctx *, int, int, char *const *);

    Field f[kMaxFields];
    int nf = 0;
    int slot0;            // the first of the call's four staging slots (Ctx::stage)
    int clock;            // row of Ctx::ht (MONORTM_HOST_TIMING), -1: an entry without phase marks
    bool flag = false;    // the kernels' error flag comes back with the output arena and is decoded (decode_flag)
    // the total optical depths O and Ctx::lastO: a MODM call leaves them resident, an RTM / scan call reads them where it finds them
    enum { O_NONE, O_LEAVES, O_READS } o_role = O_NONE;
    int o_field = -1, o_nwn = 0, o_nlay_max = 0;
    long long Ctx::*o_counter = nullptr;

    HostCall(int slot0_, int clock_ = -1) : slot0(slot0_), clock(clock_) {}
    int add(const void *in, void *out, size_t stride, Dir dir) {
        const int i = std::min(nf++, kMaxFields - 1);   // (run() refuses a call that declared more than kMaxFields)
        f[i].in = in; f[i].out = out; f[i].stride = stride; f[i].dir = dir;
        return i;
    }
    int in(const void *p, size_t per_profile) { return add(p, nullptr, per_profile, IN); }
    int in_shared(const void *p, size_t bytes) { const int i = add(p, nullptr, bytes, IN); f[i].shared = true; return i; }
    int out(void *p, size_t per_profile) { return add(nullptr, p, per_profile, OUT); }
    int inout(void *p, size_t per_profile) { return add(p, p, per_profile, INOUT); }
    int out_zeroed(void *p, size_t per_profile) { const int i = out(p, per_profile); f[i].zeroed = true; return i; }
    int out_widened(void *p, size_t elems_per_profile) { const int i = out(p, elems_per_profile * 8); f[i].widened = true; return i; }
    void leaves_O(int field, int nwn, int nlay_max) { o_role = O_LEAVES; o_field = field; o_nwn = nwn; o_nlay_max = nlay_max; }
    void reads_O(int field, int nwn, int nlay_max, long long Ctx::*counter) {
        o_role = O_READS; o_field = field; o_nwn = nwn; o_nlay_max = nlay_max; o_counter = counter;
    }

    bool absent(const Field &x) const { return x.dir == IN ? !x.in : !x.out; }
    size_t bytes(const Field &x, int n) const { return x.shared ? x.stride : (size_t)n * x.stride; }
    // the caller's array from profile p0 on (an input; host_out: an output, whose elements may be narrower than the device's)
    const char *host(int i, int p0) const { return static_cast<const char *>(f[i].in) + (f[i].shared ? 0 : (size_t)p0 * f[i].stride); }
    char *host_out(const Field &x, int p0, int real_kind) const {
        return static_cast<char *>(x.out) + (size_t)p0 * (x.widened ? x.stride / 8 * (size_t)real_kind : x.stride);
    }

    // One device's share, profiles [p0, p0 + n): returns once everything is enqueued on the context's stream; finish() completes it.
    int enqueue(Ctx *s, int g, int p0, int n, const void *pre_obj, PreFn pre, const void *launch_obj, LaunchFn launch, Pending *pd) const {
        HIPCHK(s, hipSetDevice(s->device));
        if (int rc = pre(pre_obj, s, p0, n)) return rc;
        // O straight from the preceding MODM call?  Then it is still on the device (see Ctx::lastO): no second upload
        bool resident = false;
        if (o_role == O_READS) {
            const size_t b = bytes(f[o_field], n);
            resident = s->lastO.dev && s->lastO.nprof == n && s->lastO.nwn == o_nwn && s->lastO.nlay_max == o_nlay_max && s->lastO.bytes == b &&
                       memcmp(host(o_field, p0), s->lastO.host, b) == 0;
            if (resident) (s->*o_counter)++;
        }
        // an in/out array lives in the output arena and is seeded from its piece of the input arena (move_arena's second piece)
        Arena in, out;
        size_t ioff[kMaxFields] = {0};
        int seed = -1;
        for (int i = 0; i < nf; i++) {
            if (absent(f[i])) continue;
            if (f[i].dir != OUT && !(resident && i == o_field)) ioff[i] = in.add(bytes(f[i], n));
            if (f[i].dir != IN) pd->off[i] = out.add(bytes(f[i], n));
            if (f[i].dir == INOUT) seed = i;
        }
        void *hin = nullptr, *din = nullptr, *hout = nullptr, *dout = nullptr;
        HIPCHK(s, stage_get(s, slot0, in.size, true, &hin));
        HIPCHK(s, stage_get(s, slot0 + 1, in.size, false, &din));
        HIPCHK(s, stage_get(s, slot0 + 2, out.size, true, &hout));
        HIPCHK(s, stage_get(s, slot0 + 3, out.size, false, &dout));
        char *h = static_cast<char *>(hin), *dv = static_cast<char *>(din), *dz = static_cast<char *>(dout);
        pd->hc.start(s, clock);
        char *dev[kMaxFields] = {nullptr};
        for (int i = 0; i < nf; i++) {
            if (absent(f[i])) continue;
            const bool packed = f[i].dir != OUT && !(resident && i == o_field);
            if (packed) memcpy(h + ioff[i], host(i, p0), bytes(f[i], n));
            dev[i] = f[i].dir != IN ? dz + pd->off[i] : (packed ? dv + ioff[i] : static_cast<char *>(const_cast<void *>(s->lastO.dev)));
        }
        pd->hc.mark(0);
        if (seed >= 0)
            HIPCHK(s, move_arena(din, hin, in.size, hipMemcpyHostToDevice, s->hs, nullptr, nullptr, dev[seed], h + ioff[seed],
                                 (bytes(f[seed], n) + 255) & ~size_t(255)));
        else HIPCHK(s, move_arena(din, hin, in.size, hipMemcpyHostToDevice, s->hs));
        for (int i = 0; i < nf; i++)
            if (f[i].zeroed && !absent(f[i])) HIPCHK(s, hipMemsetAsync(dev[i], 0, bytes(f[i], n), s->hs));
        if (int rc = launch(launch_obj, s, g, n, dev)) return rc;
        HIPCHK(s, move_arena(hout, dout, out.size, hipMemcpyDeviceToHost, s->hs, flag ? s->errflag : nullptr, flag ? s->errflag_host : nullptr));
        pd->hc.mark(1);
        pd->s = s; pd->p0 = p0; pd->n = n;
        pd->hout = static_cast<char *>(hout); pd->dout = dz;
        return MONORTM_OK;
    }

    // wait for the share's stream, decode the error flag where the entry asks for it, unpack into the caller's arrays
    int finish(Pending &pd) const {
        Ctx *s = pd.s;
        HIPCHK(s, hipSetDevice(s->device));
        HIPCHK(s, hipStreamSynchronize(s->hs));
        pd.hc.mark(2);
        if (flag)
            if (int rc = decode_flag(s, *s->errflag_host, s->hs)) return rc;
        for (int i = 0; i < nf; i++) {
            if (absent(f[i]) || f[i].dir == IN || f[i].zeroed) continue;
            char *dst = host_out(f[i], pd.p0, s->real_kind);
            if (f[i].widened) obs_unpack(dst, pd.hout + pd.off[i], bytes(f[i], pd.n) / 8, s->real_kind);
            else memcpy(dst, pd.hout + pd.off[i], bytes(f[i], pd.n));
        }
        pd.hc.mark(3);
        if (o_role == O_LEAVES) {
            const size_t o = pd.off[o_field];
            s->lastO.dev = pd.dout + o; s->lastO.host = pd.hout + o; s->lastO.bytes = bytes(f[o_field], pd.n);
            s->lastO.nprof = pd.n; s->lastO.nwn = o_nwn; s->lastO.nlay_max = o_nlay_max;
        }
        return MONORTM_OK;
    }

    int run_shares(Ctx *c, int nprof, const void *pre_obj, PreFn pre, const void *launch_obj, LaunchFn launch) const {
        if (nf > kMaxFields) { c->err = "HostCall: more arrays declared than kMaxFields"; return MONORTM_EARG; }
        if (c->shards.empty()) {
            Pending pd;
            if (int rc = enqueue(c, -1, 0, nprof, pre_obj, pre, launch_obj, launch, &pd)) return rc;
            return finish(pd);
        }
        const int G = (int)c->shards.size();
        std::vector<Pending> pend(G);
        int rc = MONORTM_OK;
        auto failed = [&](int r, Ctx *s) {   // the first error wins
            if (r && !rc) { rc = r; c->err = "device " + std::to_string(s->device) + ": " + s->err; }
        };
        for (int g = 0; g < G; g++) {
            int p0, n;
            shard_block(nprof, G, g, &p0, &n);
            if (n < 1) continue;
            failed(enqueue(c->shards[g], g, p0, n, pre_obj, pre, launch_obj, launch, &pend[g]), c->shards[g]);   // (pend[g].s stays null)
        }
        for (int g = 0; g < G; g++)
            if (pend[g].s) failed(finish(pend[g]), c->shards[g]);
        return rc;
    }

    // pre(s, p0, n): what the entry checks or prepares per share, before anything of it is staged; launch(s, g, n, dev): the *_dev call
    // of the share on shard g (-1: the context itself) with dev[i] the device address of the array declared as i
    template <class Pre, class Launch>
    int run(Ctx *c, int nprof, const Pre &pre, const Launch &launch) const {
        return run_shares(c, nprof, &pre, [](const void *o, Ctx *s, int p0, int n) { return (*static_cast<const Pre *>(o))(s, p0, n); }, &launch,
                          [](const void *o, Ctx *s, int g, int n, char *const *dev) { return (*static_cast<const Launch *>(o))(s, g, n, dev); });
    }
    template <class Launch>
    int run(Ctx *c, int nprof, const Launch &launch) const {
        return run(c, nprof, [](Ctx *, int, int) { return (int)MONORTM_OK; }, launch);
    }
};

}  // namespace

extern "C" {

const char *monortm_hip_last_error(void *ctx) {
    if (!ctx) return g_init_error.c_str();
    return static_cast<Ctx *>(ctx)->err.c_str();
}

int monortm_hip_init(const char *tape3_path, double v1, double v2, int icp, int real_kind, int device, void **out) {
    (void)icp;  // passed through to GET_LNFL by the reference and unused there (lnfl_mod.f90:22)
    *out = nullptr;
    if (real_kind != 8 && real_kind != 4) { g_init_error = "real_kind must be 8 (\"dbl\" build) or 4 (\"sgl\" build)"; return MONORTM_EUNSUPPORTED; }
    Ctx *c = new Ctx;
    c->real_kind = real_kind;
    auto failed = [&](int rc) { g_init_error = c->err; for (void *p : c->owned) hipFree(p); delete c; return rc; };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { c->err = "no HIP device available: the MI355X path has no CPU fallback"; return failed(MONORTM_EHIP); }
    if (device >= 0) { if (hipSetDevice(device) != hipSuccess) { c->err = "hipSetDevice failed"; return failed(MONORTM_EHIP); } }
    hipGetDevice(&c->device);
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && n > 0) c->cus = n; }
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) {
            c->phys_cap = std::max<size_t>(c->phys_cap, total_b / 8);
            c->far_cap = std::max<size_t>(c->far_cap, total_b / 32);
        } else (void)hipGetLastError();
        // the caller's say on how much device memory the dense-grid workspaces may take (they are raw hipMalloc, outside any
        // framework's caching allocator, grow on demand and are released when a later call needs less than a quarter of them):
        // MONORTM_PHYS_CAP / MONORTM_FAR_CAP in MiB; 0 = no workspace of that kind (line physics in place / far field inside lines_kernel)
        for (int k = 0; k < 2; k++)
            if (const char *e = getenv(k ? "MONORTM_FAR_CAP" : "MONORTM_PHYS_CAP")) {
                char *end = nullptr;
                const double mib = strtod(e, &end);
                if (end == e || *end != '\0' || !(mib >= 0.)) { c->err = std::string(k ? "MONORTM_FAR_CAP" : "MONORTM_PHYS_CAP") + ": not a number of MiB"; return failed(MONORTM_EARG); }
                (k ? c->far_cap : c->phys_cap) = (size_t)(mib * 1048576.);
            }
    }
    // an empty path gives a context without a line table (RTM / CALCTMR need no TAPE3)
    int rc = MONORTM_OK;
    if (tape3_path && tape3_path[0]) {
        rc = monortm::load_tape3(tape3_path, v1, v2, c->host, c->err, c->real_kind);
        c->has_lines = rc == MONORTM_OK;
    }
    if (rc) return failed(rc);
    const monortm::LineTable &h = c->host;
    DevLines &L = c->lines;
#define UP(field, vec) if ((rc = upload(c, (vec).data(), (vec).size(), &L.field))) return failed(rc)
    UP(vnu, h.vnu); UP(s0adj, h.s0adj); UP(lc, h.lc); UP(alfa, h.alfa); UP(hwhm, h.hwhm); UP(epp, h.epp);
    UP(tmpalf, h.tmpalf); UP(pshift, h.pshift); UP(sdep, h.sdep); UP(meta, h.meta); UP(brd_flg, h.brd_flg); UP(brd_dat, h.brd_dat);
#undef UP
    for (int m = 0; m <= MXMOL + 1; m++) L.mol_start[m] = h.mol_start[m];
    L.sorted_mask = 0;
    for (int m = 1; m <= MXMOL; m++) if (h.sorted[m]) L.sorted_mask |= (1ull << m);
    L.max_abs_shift = h.max_abs_shift;
    L.lc_mask = 0;
    size_t ncoupled = 0;
    for (size_t i = 0; i < h.meta.size(); i++)
        if ((h.meta[i] >> 10) & 3) { L.lc_mask |= (1ull << (h.meta[i] & 63)); ncoupled++; }
    c->lc_frac = h.meta.empty() ? 0. : (double)ncoupled / (double)h.meta.size();
    {
        double vlo = 0., vhi = 0.;
        if (!h.vnu.empty()) {
            const auto mm = std::minmax_element(h.vnu.begin(), h.vnu.end());
            vlo = *mm.first;
            vhi = *mm.second;
        }
        c->lines_per_cm = (double)h.size() / std::max(vhi - vlo, 1.0);
    }
    static const bool no_physics_pass = getenv("MONORTM_NO_PHYSICS_PASS") != nullptr;
    c->no_physics_pass = no_physics_pass;
    {   // the isotopologues the table holds per molecule (at least the first: a line without a known one reads its Doppler factor)
        int iso_max[MXMOL + 1] = {0};
        for (size_t i = 0; i < h.meta.size(); i++) {
            const int mol = (int)(h.meta[i] & 63u), iso = (int)((h.meta[i] >> 6) & 15u);
            if (mol >= 1 && mol <= MXMOL) iso_max[mol] = std::max(iso_max[mol], std::max(iso, 1));
        }
        int acc = 0;
        for (int m = 0; m < MXMOL; m++) { c->ms_slot_host[m] = acc; acc += std::min(iso_max[m + 1], 9); }
        c->ms_slot_host[MXMOL] = acc;
        if ((rc = upload(c, c->ms_slot_host, (size_t)MXMOL + 1, &c->ms_slot_base))) return failed(rc);
    }
    DevTables &t = c->tables;
#define UT(field, arr) if ((rc = upload(c, arr, sizeof(arr) / sizeof(arr[0]), &t.field))) return failed(rc)
    UT(self296, MT_SELF296); UT(self260, MT_SELF260); UT(frgn296, MT_FRGN296); UT(fco2, MT_FCO2);
    UT(n2c296, MT_N2RT296_C); UT(n2sf296, MT_N2RT296_SF); UT(n2c220, MT_N2RT220_C); UT(n2sf220, MT_N2RT220_SF);
    UT(xfac_rhu, MT_XFAC_RHU); UT(xfacco2, MT_XFACCO2); UT(tdep_bandhead, MT_TDEP_BANDHEAD);
    UT(tips_qoft, TIPS_QOFT); UT(smass, ISO_SMASS); UT(tips_isonm, TIPS_ISONM); UT(tips_offset, TIPS_OFFSET);
    UT(o3ch_x, MT_O3CH_X); UT(o3ch_y, MT_O3CH_Y); UT(o3ch_z, MT_O3CH_Z); UT(o3hh0, MT_O3HH0); UT(o3hh1, MT_O3HH1);
    UT(o3hh2, MT_O3HH2); UT(o3huv, MT_O3HUV); UT(o2f_x, MT_O2F_XO2); UT(o2f_t, MT_O2F_XO2T); UT(o2inf1, MT_O2INF1);
    UT(o2inf3, MT_O2INF3); UT(o2vis, MT_O2VIS); UT(o2fuv, MT_O2FUV); UT(n2f_272, MT_N2F_272); UT(n2f_228, MT_N2F_228);
    UT(n2f_ah2o, MT_N2F_AH2O); UT(n2f1, MT_N2F1);
#undef UT
    {   // Q(296 K) of every isotopologue, interpolated exactly like Q(T)
        std::vector<double> q296(sizeof(TIPS_QOFT) / sizeof(double) / 119);
        for (size_t i = 0; i < q296.size(); i++) q296[i] = tips_atob(296., &TIPS_QOFT[i * 119]);
        if ((rc = upload(c, q296.data(), q296.size(), &t.tips_q296))) return failed(rc);
    }
    {   // log ratios of the temperature interpolations below 820 cm-1 (DevTables::lr_*), with the device's log()
        const struct { const double *t296, *tlow; const double **out; int n; } lr[3] = {
            {t.self296, t.self260, &t.lr_self, MT_SELF296_NPT},
            {t.n2c296, t.n2c220, &t.lr_n2c, MT_N2RT296_NPT},
            {t.n2sf296, t.n2sf220, &t.lr_n2sf, MT_N2RT296_NPT}};
        for (const auto &e : lr) {
            void *p = nullptr;
            if (hipMalloc(&p, sizeof(double) * (size_t)e.n) != hipSuccess) { c->err = "hipMalloc(log-ratio table) failed"; return failed(MONORTM_EHIP); }
            c->owned.push_back(p);
            launch_logratio(e.t296, e.tlow, static_cast<double *>(p), e.n, nullptr);
            *e.out = static_cast<const double *>(p);
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { c->err = "log-ratio tables could not be formed"; return failed(MONORTM_EHIP); }
    }
    void *ef = nullptr;
    if (hipMalloc(&ef, sizeof(int)) != hipSuccess || hipMemset(ef, 0, sizeof(int)) != hipSuccess) { c->err = "hipMalloc(errflag) failed"; return failed(MONORTM_EHIP); }
    c->owned.push_back(ef);
    c->errflag = static_cast<int *>(ef);
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "device set-up failed"; return failed(MONORTM_EHIP); }  // memsets above: done before any stream uses them
    if (hipStreamCreateWithFlags(&c->hs, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->errflag_host), sizeof(int), hipHostMallocDefault) != hipSuccess) {
        c->err = "stream / pinned flag of the host-buffer entry points could not be created";
        return failed(MONORTM_EHIP);
    }
    if (const char *e = getenv("MONORTM_HOST_TIMING")) c->host_timing = e[0] == '1';
    if (getenv("MONORTM_FINISH_GENERIC")) c->opt.finish_generic = 1;  // (set, whatever its value: the default of option "finish")
    for (const char *k : {"lines_kernel", "nslice", "fair", "tile_waves", "far_levels", "ms_items", "ms_prepare", "ms_plan", "finish_mw",
#ifdef MONORTM_EXPERIMENT
                          "ms_ablate",
#endif
                         }) {
        std::string env = "MONORTM_" + std::string(k);
        for (char &ch : env) ch = (char)toupper((unsigned char)ch);
        if (const char *e = getenv(env.c_str()))
            if (set_option(c, k, e)) { c->err = env + ": " + c->err; return failed(MONORTM_EARG); }  // a mistyped switch must not run silently
    }
    if (c->host_timing && !g_timing_ctx) {  // a Fortran caller never finalizes: report at exit
        g_timing_ctx = c;
        static bool registered = false;
        if (!registered) { atexit([] { if (g_timing_ctx) print_host_timing(g_timing_ctx); }); registered = true; }
    }
    *out = c;
    return MONORTM_OK;
}

void monortm_hip_finalize(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return;
    if (!c->shards.empty()) {
        for (Ctx *sh : c->shards) monortm_hip_finalize(sh);
        delete c;
        return;
    }
    print_host_timing(c);
    if (g_timing_ctx == c) g_timing_ctx = nullptr;
    DeviceGuard guard;
    hipSetDevice(c->device);
    for (auto &e : c->events) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto &e : c->event_pool) hipEventDestroy(e);
    comm_release(c);
    if (c->hs) hipStreamDestroy(c->hs);
    if (c->errflag_host) hipHostFree(c->errflag_host);
    for (void *p : c->owned) hipFree(p);
    if (c->partial) hipFree(c->partial);
    if (c->osum) hipFree(c->osum);
    if (c->ms_scratch) hipFree(c->ms_scratch);
    if (c->ms_plan) {
#ifdef MONORTM_EXPERIMENT   // the share of waves and chunks that took the plan's fast path, over every launch of this context
        unsigned long long n[4] = {0, 0, 0, 0};
        if (getenv("MONORTM_MS_PLAN_STATS") && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(n, static_cast<unsigned long long *>(c->ms_plan) + MS_PLAN_CNT, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "ms_plan: waves %llu match %llu chunks %llu fast %llu\n", n[0], n[1], n[2], n[3]);
#endif
        hipFree(c->ms_plan);
    }
    for (void *p : c->xs_buf) hipFree(p);
    if (c->phys) hipFree(c->phys);
    if (c->far) hipFree(c->far);
    if (c->far_stream) hipStreamDestroy(c->far_stream);
    for (hipEvent_t e : c->far_ev)
        if (e) hipEventDestroy(e);
    c->mw_cache.release();
    if (c->jac_ws) hipFree(c->jac_ws);
    if (c->oe_ws) hipFree(c->oe_ws);
    if (c->oe_map) hipFree(c->oe_map);
    if (c->oe_diag) hipFree(c->oe_diag);
    if (c->oe_wmap) hipFree(c->oe_wmap);
    for (auto &ob : c->obs)
        if (ob.dev) hipFree(ob.dev);
    for (int i = 0; i < 12; i++)
        if (c->stage[i].p) {
            if (i % 2 == 0) hipHostFree(c->stage[i].p);  // even slots: pinned host arenas
            else hipFree(c->stage[i].p);
        }
    delete c;
}

int monortm_hip_init_multi(const char *tape3_path, double v1, double v2, int icp, int real_kind, int ngpu, void **out) {
    if (!out) { g_init_error = "null output pointer"; return MONORTM_EARG; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_init_error = "no HIP device available: the MI355X path has no CPU fallback"; return MONORTM_EHIP; }
    // device list: MONORTM_DEVICES="0,1,..." (an ordinal may repeat: several shards then share that device, which is how
    // the sharding is exercised on a one-GPU box) or the first ngpu visible devices; ngpu <= 0 means all of them
    std::vector<int> devs;
    if (const char *e = getenv("MONORTM_DEVICES")) {
        for (const char *q = e; *q;) {
            char *end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q) break;
            devs.push_back((int)v);
            q = (*end == ',') ? end + 1 : end;
        }
        if (ngpu > 0 && (int)devs.size() > ngpu) devs.resize(ngpu);
    }
    if (devs.empty()) {
        const int n = (ngpu <= 0) ? ndev : ngpu;
        if (n > ndev) { g_init_error = "ngpu = " + std::to_string(n) + " but only " + std::to_string(ndev) + " device(s) visible"; return MONORTM_EARG; }
        for (int g = 0; g < n; g++) devs.push_back(g);
    }
    for (int dv : devs)
        if (dv < 0 || dv >= ndev) { g_init_error = "MONORTM_DEVICES names device " + std::to_string(dv) + " outside 0.." + std::to_string(ndev - 1); return MONORTM_EARG; }
    DeviceGuard guard;  // monortm_hip_init selects each device in turn
    Ctx *m = new Ctx;
    m->real_kind = real_kind;
    for (int dv : devs) {
        void *sh = nullptr;
        const int rc = monortm_hip_init(tape3_path, v1, v2, icp, real_kind, dv, &sh);
        if (rc) {  // g_init_error holds the text
            for (Ctx *x : m->shards) monortm_hip_finalize(x);
            delete m;
            return rc;
        }
        m->shards.push_back(static_cast<Ctx *>(sh));
    }
    m->has_lines = m->shards[0]->has_lines;
    m->device = m->shards[0]->device;
    *out = m;
    return MONORTM_OK;
}

int monortm_hip_device_count(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return 0;
    return c->shards.empty() ? 1 : (int)c->shards.size();
}

int monortm_hip_tape3_probe(const char *tape3_path, double v1, double v2, long long *n_physical, long long *n_entries,
                            long long *n_coupled) {
    monortm::LineTable t;
    std::string err;
    int rc = monortm::load_tape3(tape3_path ? tape3_path : "", v1, v2, t, err);
    if (rc) {
        g_init_error = err;
        return rc;
    }
    for (int m = 0; m <= MXMOL; m++) {
        n_physical[m] = t.n_physical[m];
        n_entries[m] = (m == 0) ? (long long)t.size() : t.mol_start[m + 1] - t.mol_start[m];
        n_coupled[m] = 0;
    }
    for (size_t i = 0; i < t.meta.size(); i++)
        if ((t.meta[i] >> 10) & 3) {
            n_coupled[t.meta[i] & 63]++;
            n_coupled[0]++;
        }
    return MONORTM_OK;
}

// ---- the single output gather of a profile-sharded job (north_star), for callers without Python --------------
// RCCL is opened on first use (dlopen: a one-GPU caller never loads it, and a process that already holds a copy - torch ships
// one - keeps using that one).  Only the handful of entry points the gather needs are bound.
namespace {
struct Rccl {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Gather)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    void *init_rank = nullptr;
};
struct NcclId { char b[128]; };  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
Rccl g_rccl;
bool rccl_open(std::string &err) {
    if (g_rccl.h) return true;
    for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.h) break;
    }
    if (!g_rccl.h) {
        const char *de = dlerror();  // (one call: dlerror() clears the message it returns)
        err = std::string("RCCL cannot be loaded: ") + (de ? de : "librccl.so.1 not found");
        return false;
    }
    g_rccl.GetUniqueId = reinterpret_cast<int (*)(void *)>(dlsym(g_rccl.h, "ncclGetUniqueId"));
    g_rccl.init_rank = dlsym(g_rccl.h, "ncclCommInitRank");
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void *)>(dlsym(g_rccl.h, "ncclCommDestroy"));
    g_rccl.Gather = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, void *, hipStream_t)>(dlsym(g_rccl.h, "ncclGather"));
    g_rccl.GetErrorString = reinterpret_cast<const char *(*)(int)>(dlsym(g_rccl.h, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.init_rank || !g_rccl.CommDestroy || !g_rccl.Gather) {
        err = "RCCL lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclGather";
        dlclose(g_rccl.h);
        g_rccl = Rccl{};
        return false;
    }
    return true;
}
void comm_release(Ctx *c) {
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
}
int rccl_fail(Ctx *c, const char *what, int rc) {
    c->err = std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")";
    return MONORTM_EHIP;
}
}  // namespace

int monortm_hip_comm_unique_id(void *id128) {
    // no context yet: the reason of a failure is left where monortm_hip_last_error(NULL) finds it
    if (!id128) { g_init_error = "monortm_hip_comm_unique_id: null id buffer"; return MONORTM_EARG; }
    std::string err;
    if (!rccl_open(err)) { g_init_error = err; return MONORTM_EHIP; }
    const int rc = g_rccl.GetUniqueId(id128);
    if (rc != 0) {
        g_init_error = std::string("ncclGetUniqueId: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")";
        return MONORTM_EHIP;
    }
    return MONORTM_OK;
}

int monortm_hip_comm_init(void *ctx, int world, int rank, const void *id128) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    if (world < 1 || rank < 0 || rank >= world || !id128) { c->err = "bad world / rank / id"; return MONORTM_EARG; }
    if (!rccl_open(c->err)) return MONORTM_EHIP;
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) { g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    NcclId id;
    memcpy(id.b, id128, sizeof id.b);
    auto init = reinterpret_cast<int (*)(void **, int, NcclId, int)>(g_rccl.init_rank);
    const int rc = init(&c->comm, world, id, rank);
    if (rc != 0) { c->comm = nullptr; return rccl_fail(c, "ncclCommInitRank", rc); }
    c->comm_rank = rank;
    c->comm_world = world;
    return MONORTM_OK;
}

int monortm_hip_gather_dev(void *ctx, const void *send, size_t bytes, void *recv, int root, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->comm) { c->err = "no communicator on this context: call monortm_hip_comm_init first"; return MONORTM_EARG; }
    if (!send || root < 0 || root >= c->comm_world || (c->comm_rank == root && !recv)) { c->err = "bad gather arguments"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    const int rc = g_rccl.Gather(send, recv, bytes, /* ncclUint8 */ 1, root, c->comm, (hipStream_t)stream);
    if (rc != 0) return rccl_fail(c, "ncclGather", rc);
    return MONORTM_OK;
}

int monortm_hip_set_option(void *ctx, const char *name, const char *value) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    int rc = set_option(c, name, value);
    for (Ctx *sh : c->shards)
        if (int r = set_option(sh, name, value)) rc = r;
    return rc;
}

int monortm_hip_has_lines(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    return (c && c->has_lines) ? 1 : 0;
}

int monortm_hip_xsec_regions(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return 0;
    if (!c->shards.empty()) c = c->shards[0];
    return c->xs.nreg;
}

int monortm_hip_kat(void *ctx, int which, int n, const double *args, const double *tab119, double *out) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) c = c->shards[0];
    if (which < 1 || which > 11 || n < 1 || !args || !out || (which == 5 && !tab119)) { c->err = "bad known-answer request"; return MONORTM_EARG; }
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    double *din = nullptr, *dtab = nullptr, *dout = nullptr;
    auto run = [&]() -> int {
        HIPCHK(c, hipMalloc(&din, sizeof(double) * 4 * n));
        HIPCHK(c, hipMalloc(&dtab, sizeof(double) * 119));
        HIPCHK(c, hipMalloc(&dout, sizeof(double) * 2 * n));
        HIPCHK(c, hipMemcpy(din, args, sizeof(double) * 4 * n, hipMemcpyHostToDevice));
        if (tab119) HIPCHK(c, hipMemcpy(dtab, tab119, sizeof(double) * 119, hipMemcpyHostToDevice));
        launch_kat(which, n, din, dtab, dout, c->errflag, c->tables, nullptr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpy(out, dout, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
        return MONORTM_OK;
    };
    const int rc = run();
    hipFree(din); hipFree(dtab); hipFree(dout);  // (hipFree(nullptr) is a no-op: every exit path releases what was allocated)
    return rc ? rc : monortm_hip_check(c, nullptr);
}

long long monortm_hip_counter(void *ctx, int which) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return -1;
    if (!c->shards.empty()) {
        long long t = 0;
        for (Ctx *sh : c->shards) t += monortm_hip_counter(sh, which);
        return t;
    }
    if (which == 0) return c->o_reused;
    if (which == 1) return c->o_reused_scan;
    if (which >= 2 && which <= 7) return c->finish_launches[which - 2];
    if (which == 9) return c->finish_mw_col_launches;
    if (which >= 16 && which <= 19) return c->far_launches[which - 16];
    return -1;
}

long long monortm_hip_line_count(void *ctx, int mol) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || mol < 0 || mol > MXMOL) return -1;
    if (!c->shards.empty()) c = c->shards[0];  // every device holds the same table
    return c->host.n_physical[mol];
}

int monortm_hip_profile(void *ctx, int enable) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    c->profiling = enable & 7;
    c->prof_stride = std::max(1, enable >> 8);
    for (auto &n : c->prof_calls) n = 0;
    return MONORTM_OK;
}

int monortm_hip_kernel_time(void *ctx, int kernel, double *total_ms, long long *launches) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    if (!total_ms || !launches) { c->err = "null output pointer"; return MONORTM_EARG; }
    if (kernel < 0 || kernel > 2) { c->err = "kernel id must be 0..2"; return MONORTM_EARG; }
    for (auto &e : c->events) {
        float ms = 0.f;
        HIPCHK(c, hipEventSynchronize(e.b));
        HIPCHK(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->tot_ms[e.k] += ms;
        c->launches[e.k]++;
        c->event_pool.push_back(e.a);
        c->event_pool.push_back(e.b);
    }
    c->events.clear();
    *total_ms = c->tot_ms[kernel];
    *launches = c->launches[kernel];
    return MONORTM_OK;
}

int monortm_hip_check(void *ctx, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, c->errflag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    return decode_flag(c, flag, (hipStream_t)stream);
}

int monortm_hip_modm_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                         int nmol, const void *P, const void *T, const void *CLW, const void *WKL,
                         const void *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw, double y0res,
                         int ibrd, int ixsect, void *O, void *O_BY_MOL, void *OC, void *O_CLW, const double *wn_ends,
                         void *stream) {
    if (ixsect != 0) {
        Ctx *c = static_cast<Ctx *>(ctx);
        if (!c) return null_ctx();
        c->err = "IXSECT = 1 needs the column amounts of the cross-section molecules and an ODXSEC array: call monortm_hip_modm_xs_dev "
                 "(the reference passes them through COMMON /PATHX/ and its ODXSEC argument, src/modm.f90:24,197)";
        return MONORTM_EUNSUPPORTED;
    }
    return monortm_hip_modm_xs_dev(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw,
                                   y0res, ibrd, 0, nullptr, nullptr, O, O_BY_MOL, OC, O_CLW, wn_ends, stream);
}

int monortm_hip_xsec_tables(void *ctx, int nxs, int nreg, const double *reg, const double *temps, const double *pres_mb,
                            const long long *offs, const double *pool, long long npool) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) {
        for (Ctx *sh : c->shards)
            if (int rc = monortm_hip_xsec_tables(sh, nxs, nreg, reg, temps, pres_mb, offs, pool, npool)) { c->err = sh->err; return rc; }
        return MONORTM_OK;
    }
    if (nxs < 0 || nxs > 38 || nreg < 0 || npool < 0 || (nreg > 0 && (!reg || !temps || !pres_mb || !offs || !pool))) { c->err = "bad cross-section tables"; return MONORTM_EARG; }
    for (int r = 0; r < nreg; r++) {   // shapes the kernel relies on
        const int m = (int)reg[r * 8], npts = (int)reg[r * 8 + 3], nt = (int)reg[r * 8 + 4];
        if (m < 0 || m >= nxs || npts < 2 || nt < 1 || nt > 6 || !(reg[r * 8 + 2] > reg[r * 8 + 1]) || !(reg[r * 8 + 7] > reg[r * 8 + 6])) { c->err = "bad cross-section region"; return MONORTM_EARG; }
        for (int k = 0; k < nt; k++)
            if (offs[r * 6 + k] < 0 || offs[r * 6 + k] + npts > npool) { c->err = "cross-section spectrum outside the pool"; return MONORTM_EARG; }
    }
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());   // no kernel may still read the tables that are replaced
    for (void *p : c->xs_buf) hipFree(p);
    c->xs_buf.clear();
    c->xs = DevXsec{};
    auto up = [&](const void *src, size_t bytes, const void **dst) -> int {
        void *p = nullptr;
        HIPCHK(c, hipMalloc(&p, std::max<size_t>(bytes, 8)));
        c->xs_buf.push_back(p);
        if (bytes) HIPCHK(c, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        *dst = p;
        return MONORTM_OK;
    };
    const size_t n6 = (size_t)nreg * 6;
    int rc;
    if ((rc = up(reg, (size_t)nreg * 8 * 8, reinterpret_cast<const void **>(&c->xs.reg)))) return rc;
    if ((rc = up(temps, n6 * 8, reinterpret_cast<const void **>(&c->xs.temps)))) return rc;
    if ((rc = up(pres_mb, n6 * 8, reinterpret_cast<const void **>(&c->xs.pres)))) return rc;
    if ((rc = up(offs, n6 * 8, reinterpret_cast<const void **>(&c->xs.offs)))) return rc;
    if ((rc = up(pool, (size_t)npool * 8, reinterpret_cast<const void **>(&c->xs.pool)))) return rc;
    c->xs.nxs = nxs;
    c->xs.nreg = nreg;
    return MONORTM_OK;
}

}  // extern "C"

namespace {
// monortm_hip_modm_xs_dev, and its variant for the Jacobian entries (jac_states): odx_given - with ixsect = 1 - says that ODXSEC already
// holds the cross sections' optical depth of every state of this launch (xsec_kernel for the base state, xsec_jac_kernel for T +- h
// and P (1 +- eps), zero for the states that run without them): xsec_kernel is not launched, XAMNT is not read, and the finish kernel
// adds ODXSEC into O as ever.
int modm_dev_impl(Ctx *c, const AtmIn &atm, bool odx_given, const ModmOut &out, hipStream_t s) {
    const int nprof = atm.nprof, nwn = atm.nwn, nlay_max = atm.nlay_max, nmol = atm.nmol, ibrd = atm.ibrd, ixsect = atm.ixsect;
    if (!c->shards.empty()) return multi_only_host(c);
    if (!c->has_lines) { c->err = "this context holds no line table (created without a TAPE3 path): MODM needs one (GET_LNFL, modm.f90:187-190)"; return MONORTM_EARG; }
    if (any_null({atm.wn, atm.nlay, atm.P, atm.T, atm.CLW, atm.WKL, atm.WBRODL, atm.cntnm_fac, out.O, out.O_BY_MOL, out.OC, out.O_CLW})) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    // first / last wavenumber decide the ABSRB grid (modm.f90:180-185).  A caller that knows them passes them in
    // wn_ends (host) and the call stays asynchronous; otherwise they are fetched from device memory (one sync).
    double vends[2];
    if (atm.wn_ends) {
        vends[0] = atm.wn_ends[0];
        vends[1] = atm.wn_ends[1];
    } else {
        HIPCHK(c, hipMemcpyAsync(&vends[0], atm.wn, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&vends[1], atm.wn + (nwn > 0 ? nwn - 1 : 0), sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    int rc = check_modm_args(c, nprof, nwn, nlay_max, nmol, ibrd, ixsect, vends[1]);
    if (rc) return rc;
    ModmArgs a{};
    a.real_kind = c->real_kind;
    a.nprof = nprof; a.nwn = nwn; a.nlay_max = nlay_max; a.nmol = nmol; a.ibrd = ibrd;
    a.dvset = atm.dvset; a.sclcpl = atm.sclcpl; a.sclhw = atm.sclhw; a.y0res = atm.y0res;
    for (int i = 0; i < 7; i++) a.cntnm[i] = atm.cntnm_fac[i];
    a.wn = atm.wn; a.P = atm.P; a.T = atm.T; a.CLW = atm.CLW; a.WKL = atm.WKL; a.WBRODL = atm.WBRODL; a.nlay = atm.nlay;
    a.O = out.O; a.O_BY_MOL = out.O_BY_MOL; a.OC = out.OC; a.O_CLW = out.O_CLW; a.errflag = c->errflag;
    if (ixsect == 1) {
        if ((!atm.XAMNT && !odx_given) || !out.ODXSEC) { c->err = "IXSECT = 1: XAMNT / ODXSEC missing"; return MONORTM_EARG; }
        if (c->xs.nxs < 1) { c->err = "IXSECT = 1: no cross-section tables on this context (monortm_hip_xsec_tables)"; return MONORTM_EARG; }
        a.XAMNT = atm.XAMNT; a.ODXSEC = out.ODXSEC; a.nxs = c->xs.nxs;
    }

    // what the call launches: decided from the shape, the table's and the device's constants alone (modm_plan.hpp)
    ModmPlanIn in{};
    in.nprof = nprof; in.nwn = nwn; in.nlay_max = nlay_max; in.nmol = nmol; in.real_kind = c->real_kind; in.ibrd = ibrd; in.ixsect = ixsect;
    in.v1 = vends[0]; in.v2 = vends[1];
    in.nlines = (long long)c->host.size(); in.lines_per_cm = c->lines_per_cm; in.lc_frac = c->lc_frac; in.any_brd = c->host.any_brd;
    in.ms_nslot = c->ms_slot_host[nmol];   // slots of the molecules of this call: slot_base[nmol] pairs
    in.cus = c->cus; in.phys_cap = c->phys_cap; in.far_cap = c->far_cap;
    in.opt = c->opt;
    in.no_physics_pass = c->no_physics_pass;
    ModmPlan pl;
    const char *why = nullptr;
    if ((rc = modm_plan(in, &pl, &why))) { c->err = why; return rc; }

    HIPCHK(c, grow(&c->partial, &c->partial_elems, pl.partial_elems, (size_t)c->real_kind));   // (0 elements: one slice)
    a.nslice = pl.nslice;
    a.partial = c->partial;
    a.fair = pl.fair;
    if (pl.need_osum) {
        HIPCHK(c, grow(reinterpret_cast<void **>(&c->osum), &c->osum_elems, pl.osum_elems, sizeof(double)));
        a.osum = c->osum;
    }
    Ctx::Ev ev{};
    prof_begin(c, s, 0, ev);
    if ((rc = dense_passes(c, pl, a, s))) return rc;
    MsArgs ms = pl.ms;
    if (pl.use_ms) {
        HIPCHK(c, grow(&c->ms_scratch, &c->ms_scratch_bytes, lines_ms_scratch(ms, (long long)ms.npg * nlay_max)));
        const size_t nl4 = (std::max<size_t>(c->host.size(), 1) + 3) / 4 * 4;
        if (!c->ms_reach) {   // two bytes + one float per table line (the table does not change)
            void *p = nullptr;
            HIPCHK(c, hipMalloc(&p, 6 * nl4));
            c->owned.push_back(p);
            c->ms_reach = static_cast<unsigned short *>(p);
        }
        ms.reach = c->ms_reach;
        ms.near0 = reinterpret_cast<float *>(c->ms_reach + nl4);
        ms.scratch = c->ms_scratch;
        ms.slot_base = c->ms_slot_base;
        ms.ablate = c->opt.ms_ablate;
        ms.prepare = c->opt.ms_prepare;
        ms.plan_on = c->opt.ms_plan;
        if (ms.plan_on) {
            const size_t had = c->ms_plan_words;
            HIPCHK(c, grow(&c->ms_plan, &c->ms_plan_words, lines_ms_plan_words((long long)c->host.size(), ms.CL), sizeof(unsigned long long)));
            if (c->ms_plan_words != had) HIPCHK(c, hipMemsetAsync(c->ms_plan, 0, c->ms_plan_words * sizeof(unsigned long long), s));
            ms.plan = static_cast<unsigned long long *>(c->ms_plan);
        }
    }
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]);
    if (pl.use_ms && pl.ms_nprof < nprof) {
        // a split batch (double precision, one tile, one slice, no dense-grid workspaces): the same arguments with nprof = the whole
        // rounds for lines_ms_kernel, and shifted by those profiles for lines_kernel
        ModmArgs am = a, aw = a;
        am.nprof = pl.ms_nprof;
        const size_t st = (size_t)pl.ms_nprof * nlay_max;   // states ahead of the second part
        auto shift = [](const void *p, size_t elems) { return p ? static_cast<const void *>(static_cast<const double *>(p) + elems) : nullptr; };
        aw.nprof = nprof - pl.ms_nprof;
        aw.P = shift(a.P, st); aw.T = shift(a.T, st); aw.CLW = shift(a.CLW, st); aw.WBRODL = shift(a.WBRODL, st);
        aw.WKL = shift(a.WKL, st * nmol);
        aw.nlay = a.nlay + pl.ms_nprof;
        aw.O = const_cast<void *>(shift(a.O, st * nwn)); aw.O_CLW = const_cast<void *>(shift(a.O_CLW, st * nwn));
        aw.O_BY_MOL = const_cast<void *>(shift(a.O_BY_MOL, st * nmol * nwn));
        aw.OC = const_cast<void *>(shift(a.OC, st * MONORTM_NCONT * nwn));
        aw.osum = a.osum ? a.osum + st * nwn : nullptr;
        launch_lines_ms(am, c->lines, c->tables, ms, pl.use_brd, s);
        launch_lines(aw, c->lines, c->tables, pl.nw, pl.wpl, pl.use_brd, dim3(grid.x, (unsigned)aw.nprof, grid.z), pl.dyn_lds, s);
    } else if (pl.use_ms) launch_lines_ms(a, c->lines, c->tables, ms, pl.use_brd, s);
    else launch_lines(a, c->lines, c->tables, pl.nw, pl.wpl, pl.use_brd, grid, pl.dyn_lds, s);
    prof_end(c, s, ev);
    HIPCHK(c, hipGetLastError());
    prof_begin(c, s, 1, ev);
    if (ixsect == 1 && !odx_given) launch_xsec(a, c->xs, s);   // MONORTM_XSEC_SUB comes first (modm.f90:197); the finish kernel adds its sum into O
    a.slices_reduced = pl.slices_reduced;
    if (pl.slices_reduced) launch_reduce_slices(a, s);
    bool column = false;   // finish_mw_kernel_col served the call (launch_finish_mw chooses the layout)
    if (pl.mw) {
        const hipError_t e = launch_finish_mw(a, c->tables, vends[0], vends[1], pl.V1ABS, pl.V2ABS, pl.NPTABS, c->mw_cache, c->opt.finish_mw, c->cus, &column, s);
        if (e != hipSuccess) {
            c->err = std::string("launch_finish_mw: ") + (c->mw_cache.why ? c->mw_cache.why : hipGetErrorString(e));
            return c->mw_cache.why ? MONORTM_EUNSUPPORTED : MONORTM_EHIP;
        }
    } else HIPCHK(c, launch_finish(a, c->tables, pl.V1ABS, pl.V2ABS, pl.NPTABS, pl.csize, pl.high, pl.par, pl.fin_threads, pl.fin_lds, pl.lds_sets, s));
    c->finish_launches[pl.finish_variant]++;
    if (column) c->finish_mw_col_launches++;
    prof_end(c, s, ev);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}
}  // namespace

extern "C" {

int monortm_hip_modm_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                            int nmol, const void *P, const void *T, const void *CLW, const void *WKL,
                            const void *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw, double y0res,
                            int ibrd, int ixsect, const void *XAMNT, void *ODXSEC, void *O, void *O_BY_MOL, void *OC,
                            void *O_CLW, const double *wn_ends, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT, .wn_ends = wn_ends};
    const ModmOut out{.ODXSEC = ODXSEC, .O = O, .O_BY_MOL = O_BY_MOL, .OC = OC, .O_CLW = O_CLW};
    return modm_dev_impl(c, atm, false, out, (hipStream_t)stream);
}

int monortm_hip_rtm_dev(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                        int iout, const void *T, const void *TZ, const void *O, void *tmpsfc, const void *emiss,
                        const void *reflc, void *RUP, void *RDN, void *TRTOT, void *RAD, void *TB, void *TMR,
                        void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    hipStream_t s = (hipStream_t)stream;
    if (!wn || !nlay || !irt || !T || !TZ || !O || !tmpsfc || !emiss || !reflc || !RUP || !RDN || !TRTOT || !RAD || !TB) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    if (nprof < 1 || nwn < 1 || nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc};
    RtmArgs a{};
    rtm_args(a, atm, sfc, O);
    a.real_kind = c->real_kind; a.iout = iout;
    a.tmpsfc = tmpsfc; a.RUP = RUP; a.RDN = RDN; a.TRTOT = TRTOT; a.RAD = RAD; a.TB = TB; a.TMR = TMR;
    Ctx::Ev ev{};
    prof_begin(c, s, 2, ev);
    launch_rtm(a, s);
    prof_end(c, s, ev);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}


int monortm_hip_modm(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                     int nmol, const void *P, const void *T, const void *CLW, const void *WKL,
                     const void *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd,
                     int ixsect, void *O, void *O_BY_MOL, void *OC, void *O_CLW) {
    if (ixsect != 0) {
        Ctx *c = static_cast<Ctx *>(ctx);
        if (!c) return null_ctx();
        c->err = "IXSECT = 1 needs the column amounts of the cross-section molecules and an ODXSEC array: call monortm_hip_modm_xs";
        return MONORTM_EUNSUPPORTED;
    }
    return monortm_hip_modm_xs(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                               ibrd, 0, nullptr, nullptr, O, O_BY_MOL, OC, O_CLW);
}

int monortm_hip_modm_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max,
                        int nmol, const void *P, const void *T, const void *CLW, const void *WKL,
                        const void *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd,
                        int ixsect, const void *XAMNT, void *ODXSEC, void *O, void *O_BY_MOL, void *OC, void *O_CLW) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const bool multi = !c->shards.empty();
    if (multi && (!nlay || !P || !T || !CLW || !WKL || !WBRODL || !O || !O_BY_MOL || !OC || !O_CLW || nprof < 1 || nwn < 1 || nlay_max < 1 || nmol < 1)) {
        c->err = "bad or null argument";
        return MONORTM_EARG;
    }
    const bool xs = ixsect == 1;
    const size_t d = (size_t)c->real_kind, l = (size_t)nlay_max * d, w = l * nwn;
    const int nxs = (multi ? c->shards[0] : c)->xs.nxs;
    HostCall hc(0, 0);
    hc.flag = true;
    const int i_wn = hc.in_shared(wn, nwn * sizeof(double)), i_nl = hc.in(nlay, sizeof(int)), i_P = hc.in(P, l), i_T = hc.in(T, l),
              i_C = hc.in(CLW, l), i_W = hc.in(WKL, l * nmol), i_B = hc.in(WBRODL, l), i_XA = hc.in(xs ? XAMNT : nullptr, l * nxs);
    const int o_O = hc.out(O, w), o_OM = hc.out(O_BY_MOL, w * nmol), o_OC = hc.out(OC, w * MONORTM_NCONT), o_OL = hc.out(O_CLW, w),
              o_OX = hc.out(xs ? ODXSEC : nullptr, w);
    hc.leaves_O(o_O, nwn, nlay_max);
    // every share is checked on its own device's context, before anything of it is staged
    auto pre = [&](Ctx *s, int p0, int n) -> int {
        if (!wn || !nlay || !P || !T || !CLW || !WKL || !WBRODL || !cntnm_fac || !O || !O_BY_MOL || !OC || !O_CLW) { s->err = "null array argument"; return MONORTM_EARG; }
        if (n < 1 || nwn < 1 || nlay_max < 1 || nmol < 1) { s->err = "bad nprof/nwn/nlay_max/nmol"; return MONORTM_EARG; }
        for (int i = 1; i < nwn; i++)
            if (!(wn[i] >= wn[i - 1])) { s->err = "wavenumbers must be ascending (the reference takes v1 = wn(1), v2 = wn(nwn), modm.f90:180-181)"; return MONORTM_EARG; }
        // dvset /= 0: what the kernels rely on is the nearest grid index within +-1 (line_records) and the continuum at V1 + i dvset
        // as the reference's own CONTNM call places it - so the bound is on the cumulative drift, not on consecutive differences: the
        // reference's "sgl" driver forms WN(J) = V1 + (J-1)*DVSET with a REAL*4 product (src/monortm_sub.F90:287), which moves
        // point J by up to 6e-8 J DVSET
        if (dvset != 0.)
            for (int i = 1; i < nwn; i++)
                if (!(std::fabs(wn[i] - (wn[0] + i * dvset)) <= 0.25 * std::fabs(dvset))) { s->err = "dvset /= 0 promises the grid wn[i] = wn[0] + i dvset (COMMON /MANE/ DVSET of the reference driver)"; return MONORTM_EARG; }
        for (int p = p0; p < p0 + n; p++)
            if (nlay[p] < 1 || nlay[p] > nlay_max) { s->err = "nlay[p] outside 1..nlay_max"; return MONORTM_EARG; }
        s->lastO.dev = nullptr;  // before any arena can move or fail to regrow: nothing may point into a freed arena afterwards
        s->lastO.host = nullptr;
        if (xs && (!XAMNT || !ODXSEC || s->xs.nxs < 1)) { s->err = "IXSECT = 1: XAMNT / ODXSEC / cross-section tables missing"; return MONORTM_EARG; }
        return MONORTM_OK;
    };
    return hc.run(c, nprof, pre, [&](Ctx *s, int, int n, char *const *dv) {
        const double ends[2] = {wn[0], wn[nwn - 1]};
        return monortm_hip_modm_xs_dev(s, n, nwn, (double *)dv[i_wn], dvset, (int *)dv[i_nl], nlay_max, nmol, dv[i_P], dv[i_T], dv[i_C], dv[i_W],
                                       dv[i_B], cntnm_fac, sclcpl, sclhw, y0res, ibrd, ixsect, dv[i_XA], dv[o_OX], dv[o_O], dv[o_OM], dv[o_OC],
                                       dv[o_OL], ends, s->hs);
    });
}

int monortm_hip_rtm(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                    int iout, const void *T, const void *TZ, const void *O, void *tmpsfc, const void *emiss,
                    const void *reflc, void *RUP, void *RDN, void *TRTOT, void *RAD, void *TB, void *TMR) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    if (!c->shards.empty() && (!nlay || !irt || !T || !TZ || !O || !tmpsfc || !emiss || !reflc || !RUP || !RDN || !TRTOT || !RAD || !TB ||
                               nprof < 1 || nwn < 1 || nlay_max < 1)) {
        c->err = "bad or null argument";
        return MONORTM_EARG;
    }
    const size_t d = (size_t)c->real_kind, l = (size_t)nlay_max * d, v = (size_t)nwn * d;
    HostCall hc(4, 1);
    const int i_wn = hc.in_shared(wn, nwn * sizeof(double)), i_nl = hc.in(nlay, sizeof(int)), i_irt = hc.in(irt, sizeof(int)), i_T = hc.in(T, l),
              i_TZ = hc.in(TZ, l + d), i_O = hc.in(O, l * nwn), i_em = hc.in(emiss, v), i_rf = hc.in(reflc, v), io_ts = hc.inout(tmpsfc, d);
    // TB of a call with iout /= 1: zeroed on the device, the caller's array is left alone
    const int o_up = hc.out(RUP, v), o_dn = hc.out(RDN, v), o_tr = hc.out(TRTOT, v), o_rad = hc.out(RAD, v),
              o_tb = iout == 1 ? hc.out(TB, v) : hc.out_zeroed(TB, v), o_tmr = hc.out(TMR, v);
    hc.reads_O(i_O, nwn, nlay_max, &Ctx::o_reused);
    auto pre = [&](Ctx *s, int p0, int n) -> int {
        if (!wn || !nlay || !irt || !T || !TZ || !O || !tmpsfc || !emiss || !reflc || !RUP || !RDN || !TRTOT || !RAD || !TB) { s->err = "null array argument"; return MONORTM_EARG; }
        for (int p = p0; p < p0 + n; p++)
            if (nlay[p] < 1 || nlay[p] > nlay_max) { s->err = "nlay[p] outside 1..nlay_max"; return MONORTM_EARG; }
        if (n < 1 || nwn < 1 || nlay_max < 1) { s->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
        return MONORTM_OK;
    };
    return hc.run(c, nprof, pre, [&](Ctx *s, int, int n, char *const *dv) {
        return monortm_hip_rtm_dev(s, n, nwn, (double *)dv[i_wn], (int *)dv[i_nl], nlay_max, (int *)dv[i_irt], iout, dv[i_T], dv[i_TZ], dv[i_O],
                                   dv[io_ts], dv[i_em], dv[i_rf], dv[o_up], dv[o_dn], dv[o_tr], dv[o_rad], dv[o_tb], dv[o_tmr], s->hs);
    });
}

// ---- path scans ---------------------------------------------------------------------------------
int monortm_hip_rtm_scan_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                             int iout, const void *T, const void *TZ, const void *O, const void *path, void *tmpsfc, int sfc_per_path,
                             const void *emiss, const void *reflc, void *RUP, void *RDN, void *TRTOT, void *RAD, void *TB, void *TMR,
                             void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    hipStream_t s = (hipStream_t)stream;
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, irt, T, TZ, O, path, tmpsfc, emiss, reflc, RUP, RDN, TRTOT, RAD, TB})) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    RtmScanArgs a{};
    rtm_args(a, atm, sfc, O);
    scan_args(a, scan);
    a.real_kind = c->real_kind; a.iout = iout;
    a.tmpsfc = tmpsfc; a.RUP = RUP; a.RDN = RDN; a.TRTOT = TRTOT; a.RAD = RAD; a.TB = TB; a.TMR = TMR;
    a.errflag = c->errflag;
    Ctx::Ev ev{};
    prof_begin(c, s, 2, ev);
    launch_rtm_scan(a, s);
    prof_end(c, s, ev);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

int monortm_hip_rtm_scan(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt, int iout,
                         const void *T, const void *TZ, const void *O, const void *path, void *tmpsfc, int sfc_per_path, const void *emiss,
                         const void *reflc, void *RUP, void *RDN, void *TRTOT, void *RAD, void *TB, void *TMR) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, irt, T, TZ, O, path, tmpsfc, emiss, reflc, RUP, RDN, TRTOT, RAD, TB})) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    // the whole call's nlay and factors before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    const size_t d = (size_t)c->real_kind, l = (size_t)nlay_max * d, vo = (size_t)nwn * npath * d, vs = sfc_per_path ? vo : (size_t)nwn * d;
    HostCall hc(4, 2);
    const int i_wn = hc.in_shared(wn, nwn * sizeof(double)), i_nl = hc.in(nlay, sizeof(int)), i_irt = hc.in(irt, sizeof(int)), i_T = hc.in(T, l),
              i_TZ = hc.in(TZ, l + d), i_O = hc.in(O, l * nwn), i_f = hc.in(path, l * npath), i_em = hc.in(emiss, vs), i_rf = hc.in(reflc, vs),
              io_ts = hc.inout(tmpsfc, d);
    // TB of a call with iout /= 1: zeroed on the device, the caller's array is left alone
    const int o_up = hc.out(RUP, vo), o_dn = hc.out(RDN, vo), o_tr = hc.out(TRTOT, vo), o_rad = hc.out(RAD, vo),
              o_tb = iout == 1 ? hc.out(TB, vo) : hc.out_zeroed(TB, vo), o_tmr = hc.out(TMR, vo);
    hc.reads_O(i_O, nwn, nlay_max, &Ctx::o_reused_scan);
    return hc.run(c, nprof, [&](Ctx *s, int, int n, char *const *dv) {
        return monortm_hip_rtm_scan_dev(s, n, npath, nwn, (double *)dv[i_wn], (int *)dv[i_nl], nlay_max, (int *)dv[i_irt], iout, dv[i_T], dv[i_TZ],
                                        dv[i_O], dv[i_f], dv[io_ts], sfc_per_path, dv[i_em], dv[i_rf], dv[o_up], dv[o_dn], dv[o_tr], dv[o_rad],
                                        dv[o_tb], dv[o_tmr], s->hs);
    });
}

}  // extern "C"

// ---- measurement operators: their checks and device tables ------------------------------------------------
namespace {
constexpr int kObsMaxViews = 65535, kObsMaxChan = 65536;
constexpr size_t kObsMaxTable = size_t(1) << 26;   // entries of the per-block membership table (256 MB of int)

Ctx::Obs *obs_find(Ctx *c, int handle) {
    if (handle <= 0) return nullptr;
    Ctx::Obs &ob = c->obs[handle % Ctx::kMaxObs];
    return ob.handle == handle ? &ob : nullptr;
}
int obs_bad_handle(Ctx *c) {
    c->err = "obs: not a handle of this context (never created here, or destroyed)";
    return MONORTM_EARG;
}
// the handle's operator, and that the call's npath and nwn are the operator's
int obs_for_call(Ctx *c, int handle, int npath, int nwn, Ctx::Obs **out) {
    Ctx::Obs *ob = obs_find(c, handle);
    if (!ob) return obs_bad_handle(c);
    if (ob->npath != npath || ob->nwn != nwn) {
        c->err = "the measurement operator was created for npath = " + std::to_string(ob->npath) + ", nwn = " + std::to_string(ob->nwn) +
                 "; the call has npath = " + std::to_string(npath) + ", nwn = " + std::to_string(nwn);
        return MONORTM_EARG;
    }
    *out = ob;
    return MONORTM_OK;
}

// everything monortm_hip_obs_create refuses, on host arrays
int obs_check(Ctx *c, int npath, int nwn, int nview, int nchan, const int *view_start, const double *wpath, const int *chan,
              const double *wchan) {
    if (!view_start || !wpath || !chan || !wchan) { c->err = "null array argument"; return MONORTM_EARG; }
    if (npath < 1 || npath > kScanMaxPaths) { c->err = "npath outside 1.." + std::to_string(kScanMaxPaths); return MONORTM_EARG; }
    if (nwn < 1 || nwn > 80000) { c->err = "nwn outside 1..80000 (NWNMX, RTMmono.f90:10)"; return MONORTM_EARG; }
    if (nview < 1 || nview > kObsMaxViews) { c->err = "nview outside 1.." + std::to_string(kObsMaxViews); return MONORTM_EARG; }
    if (nchan < 1 || nchan > kObsMaxChan) { c->err = "nchan outside 1.." + std::to_string(kObsMaxChan); return MONORTM_EARG; }
    if ((size_t)((nwn + 63) / 64) * (size_t)(nchan + 1) > kObsMaxTable) { c->err = "nwn / 64 x nchan exceeds the membership table's bound (2^26 entries)"; return MONORTM_EARG; }
    if (view_start[0] != 0 || view_start[nview] != npath) { c->err = "view_start[0] must be 0 and view_start[nview] must be npath"; return MONORTM_EARG; }
    for (int v = 0; v < nview; v++)
        if (view_start[v + 1] < view_start[v]) { c->err = "view_start must not decrease (view " + std::to_string(v) + ")"; return MONORTM_EARG; }
    for (int j = 0; j < npath; j++)
        if (!std::isfinite(wpath[j])) { c->err = "wpath[" + std::to_string(j) + "] is not finite"; return MONORTM_EARG; }
    for (int i = 0; i < nwn; i++) {
        if (chan[i] < -1 || chan[i] >= nchan) { c->err = "chan[" + std::to_string(i) + "] outside -1..nchan-1"; return MONORTM_EARG; }
        if (!std::isfinite(wchan[i])) { c->err = "wchan[" + std::to_string(i) + "] is not finite"; return MONORTM_EARG; }
    }
    return MONORTM_OK;
}

// One device's copy of a checked operator: wpath, the members' weights, view_start, and per block of 64 wavenumbers the members of every
// channel in ascending wavenumber (mstart [nblk][nchan + 1] into mlane / mw) - what rtm_obs_jac_kernel's owner lanes walk.
int obs_upload(Ctx *c, Ctx::Obs &ob, const int *view_start, const double *wpath, const int *chan, const double *wchan) {
    const int nblk = (ob.nwn + 63) / 64, nchan = ob.nchan;
    std::vector<int> mstart((size_t)nblk * (nchan + 1)), mlane;
    std::vector<double> mw;
    std::vector<int> cnt(nchan + 1);
    for (int b = 0; b < nblk; b++) {
        const int i0 = b * 64, i1 = std::min(ob.nwn, i0 + 64);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int i = i0; i < i1; i++)
            if (chan[i] >= 0) cnt[chan[i] + 1]++;
        int *ms = mstart.data() + (size_t)b * (nchan + 1);
        ms[0] = (int)mlane.size();
        for (int ch = 0; ch < nchan; ch++) ms[ch + 1] = ms[ch] + cnt[ch + 1];
        mlane.resize(ms[nchan]);
        mw.resize(ms[nchan]);
        std::vector<int> fillp(ms, ms + nchan);
        for (int i = i0; i < i1; i++)   // ascending wavenumber within every channel
            if (chan[i] >= 0) {
                const int at = fillp[chan[i]]++;
                mlane[at] = i - i0;
                mw[at] = wchan[i];
            }
    }
    const size_t nm = std::max<size_t>(mlane.size(), 1);
    Arena ar;
    const size_t o_wp = ar.add(ob.npath * sizeof(double)), o_mw = ar.add(nm * sizeof(double)), o_vs = ar.add((ob.nview + 1) * sizeof(int)),
                 o_ms = ar.add(mstart.size() * sizeof(int)), o_ml = ar.add(nm * sizeof(int));
    std::vector<char> h(ar.size, 0);
    memcpy(h.data() + o_wp, wpath, ob.npath * sizeof(double));
    if (!mw.empty()) memcpy(h.data() + o_mw, mw.data(), mw.size() * sizeof(double));
    memcpy(h.data() + o_vs, view_start, (ob.nview + 1) * sizeof(int));
    memcpy(h.data() + o_ms, mstart.data(), mstart.size() * sizeof(int));
    if (!mlane.empty()) memcpy(h.data() + o_ml, mlane.data(), mlane.size() * sizeof(int));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(&ob.dev, ar.size));
    if (hipMemcpy(ob.dev, h.data(), ar.size, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(ob.dev);
        ob.dev = nullptr;
        c->err = "monortm_hip_obs_create: the copy of the operator's tables to the device failed";
        return MONORTM_EHIP;
    }
    const char *d = static_cast<const char *>(ob.dev);
    ob.wpath = reinterpret_cast<const double *>(d + o_wp);
    ob.mw = reinterpret_cast<const double *>(d + o_mw);
    ob.view_start = reinterpret_cast<const int *>(d + o_vs);
    ob.mstart = reinterpret_cast<const int *>(d + o_ms);
    ob.mlane = reinterpret_cast<const int *>(d + o_ml);
    return MONORTM_OK;
}

template <class Args>   // RtmObsJacArgs, RtmObsArgs
void obs_args(Args &a, const Ctx::Obs &ob) {
    a.nview = ob.nview; a.nchan = ob.nchan;
    a.view_start = ob.view_start; a.wpath = ob.wpath; a.mstart = ob.mstart; a.mlane = ob.mlane; a.mw = ob.mw;
}

// ---- the inputs of the Jacobian and measurement host entries, declared in ONE place ------------------------------------------------
// The index of every input among the call's arrays (HostCall), -1: none (the entry has no such argument, or it is null where it may be).
struct HostIn {
    int wn, nlay, irt, P, T, CLW, WKL, WBRODL, XAMNT, TZ, O, path, tmpsfc, emiss, reflc;
};
// O: the optical depths an entry is handed (null: it runs MODM itself, and O is among the outputs it declares)
HostIn declare_inputs(HostCall &hc, const Ctx *c, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, const void *O) {
    const size_t d = (size_t)c->real_kind, l = (size_t)atm.nlay_max * d, vs = (size_t)atm.nwn * (scan.sfc_per_path ? scan.npath : 1) * d;
    auto in = [&](const void *p, size_t per_profile) { return p ? hc.in(p, per_profile) : -1; };
    HostIn ix;
    ix.wn = hc.in_shared(atm.wn, atm.nwn * sizeof(double)); ix.nlay = in(atm.nlay, sizeof(int)); ix.irt = in(sfc.irt, sizeof(int));
    ix.P = in(atm.P, l); ix.T = in(atm.T, l); ix.CLW = in(atm.CLW, l); ix.WKL = in(atm.WKL, l * atm.nmol); ix.WBRODL = in(atm.WBRODL, l);
    ix.XAMNT = in(atm.ixsect == 1 ? atm.XAMNT : nullptr, l * ctx_nxs(c));
    ix.TZ = in(sfc.TZ, l + d); ix.O = in(O, l * atm.nwn); ix.path = in(scan.path, l * scan.npath);
    ix.tmpsfc = in(sfc.tmpsfc, d); ix.emiss = in(sfc.emiss, vs); ix.reflc = in(sfc.reflc, vs);
    return ix;
}
// The groups of one share on its device: n profiles at the device addresses of the declared arrays, the grid's ends from the host's wn
struct Share {
    AtmIn atm;
    SfcIn sfc;
    ScanIn scan;
    const void *O = nullptr;
    double ends[2] = {0., 0.};
    Share(const HostIn &ix, char *const *dv, int n, const AtmIn &h_atm, const SfcIn &h_sfc, const ScanIn &h_scan)
        : atm(h_atm), sfc(h_sfc), scan(h_scan) {
        auto at = [&](int i) -> const void * { return i < 0 ? nullptr : dv[i]; };
        atm.nprof = n;
        atm.wn = static_cast<const double *>(at(ix.wn)); atm.nlay = static_cast<const int *>(at(ix.nlay));
        atm.P = at(ix.P); atm.T = at(ix.T); atm.CLW = at(ix.CLW); atm.WKL = at(ix.WKL); atm.WBRODL = at(ix.WBRODL); atm.XAMNT = at(ix.XAMNT);
        ends[0] = h_atm.wn[0]; ends[1] = h_atm.wn[h_atm.nwn - 1];
        atm.wn_ends = ends;
        sfc.irt = static_cast<const int *>(at(ix.irt)); sfc.TZ = at(ix.TZ); sfc.tmpsfc = at(ix.tmpsfc); sfc.emiss = at(ix.emiss); sfc.reflc = at(ix.reflc);
        scan.path = at(ix.path);
        O = at(ix.O);
    }
    Share(const Share &) = delete;   // (atm.wn_ends points into the object)
    Share &operator=(const Share &) = delete;
};

// ---- the adjoints of RTM on given optical depths O (monortm_hip_rtm_jac_dev, _rtm_scan_jac_dev, _rtm_obs_jac_dev) ---------------------
int rtm_jac_dev_impl(Ctx *c, const AtmIn &atm, const SfcIn &sfc, const void *O, const JacOut &out, hipStream_t s) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (any_null({atm.wn, atm.nlay, sfc.irt, atm.T, sfc.TZ, O, sfc.tmpsfc, sfc.emiss, sfc.reflc, out.RAD, out.TB, out.K_O, out.K_T, out.K_TZ, out.K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rcq = check_quantity(c, sfc.quantity)) return rcq;
    if (atm.nprof < 1 || atm.nprof > 65535 || atm.nwn < 1 || atm.nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    RtmJacArgs a{};
    adjoint_args(a, atm, sfc, O, out);
    a.real_kind = c->real_kind;
    a.RAD = out.RAD; a.TB = out.TB; a.K_O = out.K_O;
    launch_rtm_jac(a, false, s);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

int rtm_scan_jac_dev_impl(Ctx *c, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, const void *O, const JacOut &out, hipStream_t s) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (any_null({atm.wn, atm.nlay, sfc.irt, atm.T, sfc.TZ, O, scan.path, sfc.tmpsfc, sfc.emiss, sfc.reflc, out.RAD, out.TB, out.K_T, out.K_TZ, out.K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rcq = check_quantity(c, sfc.quantity)) return rcq;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (atm.nprof > 65535) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    RtmScanJacArgs a{};
    adjoint_args(a, atm, sfc, O, out);
    scan_args(a, scan);
    a.real_kind = c->real_kind;
    a.RAD = out.RAD; a.TB = out.TB; a.K_O = out.K_O; a.K_PATH = out.K_PATH;
    a.errflag = c->errflag;
    launch_rtm_scan_jac(a, false, s);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

// out_kind: the element size of the outputs - the host entry of a real_kind = 4 context has the kernel accumulate in double and rounds
// once, when it unpacks
int rtm_obs_jac_dev_impl(Ctx *c, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, const void *O, int obs, const JacOut &out, int out_kind,
                         hipStream_t s) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (any_null({atm.wn, atm.nlay, sfc.irt, atm.T, sfc.TZ, O, scan.path, sfc.tmpsfc, sfc.emiss, sfc.reflc, out.Y, out.K_T, out.K_TZ, out.K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rcq = check_quantity(c, sfc.quantity)) return rcq;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (atm.nprof > 65535) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, scan.npath, atm.nwn, &ob)) return rc;
    if (int rcd = check_device(c)) return rcd;
    RtmObsJacArgs a{};
    adjoint_args(a, atm, sfc, O, out);
    scan_args(a, scan);
    obs_args(a, *ob);
    a.real_kind = c->real_kind;
    a.Y = out.Y;
    a.errflag = c->errflag;
    launch_rtm_obs_jac(a, false, out_kind, s);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

// ---- the full Jacobians (monortm_hip_jacobian_xs_dev, _scan_jacobian_xs_dev, _obs_jacobian_xs_dev), written once ------------------------
// MODM of the base and the 2 (1 + njac) perturbed states ONCE (jac_states), then ONE launch of the family's adjoint, chained with the
// states' differences: along the profile's own path, along every path of a scan, or contracted per measurement.
enum JacFamily { JAC_PLAIN, JAC_SCAN, JAC_OBS };
const char *const kJacEntry[3] = {"monortm_hip_jacobian", "monortm_hip_scan_jacobian", "monortm_hip_obs_jacobian"};
// the pointers a family requires (K_O and K_PATH are optional; K_W may be null with njac = 0: jac_check_mol)
bool jac_full_null(JacFamily fam, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, const JacOut &out) {
    if (any_null({atm.wn, atm.nlay, atm.P, atm.T, atm.CLW, atm.WKL, atm.WBRODL, atm.cntnm_fac, sfc.irt, sfc.TZ, sfc.tmpsfc, sfc.emiss, sfc.reflc,
                  out.O, out.K_T, out.K_TZ, out.K_CLW, out.K_SFC}))
        return true;
    if (fam != JAC_PLAIN && !scan.path) return true;
    return fam == JAC_OBS ? !out.Y : any_null({out.RAD, out.TB});
}
int jac_full(Ctx *c, JacFamily fam, const AtmIn &atm, const SfcIn &sfc, const JacReq &jq, const ScanIn &scan, int obs, const JacOut &out,
             hipStream_t s) {
    if (int rc = jac_full_check(c, kJacEntry[fam], jac_full_null(fam, atm, sfc, scan, out), atm, sfc.quantity, jq, out.K_W)) return rc;
    if (fam != JAC_PLAIN)
        if (int rc = scan_check_args(c, atm, scan)) return rc;
    Ctx::Obs *ob = nullptr;
    if (fam == JAC_OBS)
        if (int rc = obs_for_call(c, obs, scan.npath, atm.nwn, &ob)) return rc;
    if (int rcd = check_device(c)) return rcd;
    double *xO = nullptr;
    size_t st = 0;
    if (int rc = jac_states(c, atm, jq, out.O, s, &xO, &st)) return rc;
    if (fam == JAC_PLAIN) {
        RtmJacArgs a{};
        adjoint_args(a, atm, sfc, out.O, out);
        jac_chain_args(a, c, jq.njac, out.K_W, out.K_CLW, xO, st);
        a.RAD = out.RAD; a.TB = out.TB; a.K_O = out.K_O;
        launch_rtm_jac(a, true, s);
    } else if (fam == JAC_SCAN) {
        RtmScanJacArgs a{};
        adjoint_args(a, atm, sfc, out.O, out);
        scan_args(a, scan);
        jac_chain_args(a, c, jq.njac, out.K_W, out.K_CLW, xO, st);
        a.RAD = out.RAD; a.TB = out.TB; a.K_O = out.K_O; a.K_PATH = out.K_PATH;
        a.errflag = c->errflag;
        launch_rtm_scan_jac(a, true, s);
    } else {
        RtmObsJacArgs a{};
        adjoint_args(a, atm, sfc, out.O, out);
        scan_args(a, scan);
        obs_args(a, *ob);
        jac_chain_args(a, c, jq.njac, out.K_W, out.K_CLW, xO, st);
        a.Y = out.Y;
        a.errflag = c->errflag;
        launch_rtm_obs_jac(a, true, 8, s);
    }
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

// ---- the forward measurement operator: channel- and beam-averaged scans ------------------------------
int obs_check_quantity(Ctx *c, int quantity) {
    if (quantity < 0 || quantity > 2) { c->err = "quantity must be 0 (RAD), 1 (TB) or 2 (band TB)"; return MONORTM_EARG; }
    return MONORTM_OK;
}
// the channels' nominal wavenumbers of a host call (quantity 2 only): all of them, before anything is staged
int obs_check_vcen(Ctx *c, int quantity, const double *vcen, int nchan) {
    if (quantity != 2) return MONORTM_OK;
    if (!vcen) { c->err = "quantity 2 (band TB) needs vcen [nchan]"; return MONORTM_EARG; }
    for (int i = 0; i < nchan; i++)
        if (!(vcen[i] > 0. && std::isfinite(vcen[i]))) { c->err = "vcen[" + std::to_string(i) + "] is not a finite wavenumber > 0"; return MONORTM_EARG; }
    return MONORTM_OK;
}

// monortm_hip_rtm_obs_dev with the element size of Y as an argument: the host entry of a real_kind = 4 context has the kernel accumulate
// (and convert to the band temperature) in double and rounds once, when it unpacks
int rtm_obs_dev_impl(Ctx *c, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, const void *O, int obs, const double *vcen, void *Y,
                     int out_kind, hipStream_t s) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (any_null({atm.wn, atm.nlay, sfc.irt, atm.T, sfc.TZ, O, scan.path, sfc.tmpsfc, sfc.emiss, sfc.reflc, Y})) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rcq = obs_check_quantity(c, sfc.quantity)) return rcq;
    if (sfc.quantity == 2 && !vcen) { c->err = "quantity 2 (band TB) needs vcen [nchan]"; return MONORTM_EARG; }
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (atm.nprof > 65535) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, scan.npath, atm.nwn, &ob)) return rc;
    if (int rcd = check_device(c)) return rcd;
    RtmObsArgs a{};
    rtm_args(a, atm, sfc, O);
    scan_args(a, scan);
    obs_args(a, *ob);
    a.quantity = sfc.quantity; a.real_kind = c->real_kind; a.tmpsfc = sfc.tmpsfc;
    a.vcen = sfc.quantity == 2 ? vcen : nullptr;
    a.Y = Y;
    a.errflag = c->errflag;
    launch_rtm_obs(a, out_kind, s);
    HIPCHK(c, hipGetLastError());
    return MONORTM_OK;
}

// monortm_hip_obs_dev likewise: ONE MODM pass into the caller's O (the MODM outputs the operator does not use go to the context's
// workspace, grown on demand and kept), then ONE launch of the forward kernel
int obs_dev_impl(Ctx *c, const AtmIn &atm, const SfcIn &sfc, const ScanIn &scan, int obs, const double *vcen, void *O, void *Y, int out_kind,
                 hipStream_t s) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (any_null({atm.wn, atm.nlay, atm.P, atm.T, atm.CLW, atm.WKL, atm.WBRODL, atm.cntnm_fac, sfc.irt, sfc.TZ, sfc.tmpsfc, sfc.emiss, sfc.reflc,
                  scan.path, O, Y})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rcq = obs_check_quantity(c, sfc.quantity)) return rcq;
    if (sfc.quantity == 2 && !vcen) { c->err = "quantity 2 (band TB) needs vcen [nchan]"; return MONORTM_EARG; }
    if (atm.nmol < 7 || atm.nmol > MXMOL) { c->err = "nmol must be 7..39 (LINES reads WK(1:7), modm.f90:313)"; return MONORTM_EARG; }
    if (atm.nprof < 1 || atm.nprof > 65535 || atm.nwn < 1 || atm.nlay_max < 1) { c->err = "bad nprof/nwn/nlay_max"; return MONORTM_EARG; }
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, scan.npath, atm.nwn, &ob)) return rc;
    if (int rcd = check_device(c)) return rcd;
    const size_t st = (size_t)atm.nprof * atm.nlay_max * atm.nwn * (size_t)c->real_kind;   // bytes of one [nprof][nlay_max][nwn] array
    Arena ws;
    const size_t w_OM = ws.add(st * atm.nmol), w_OC = ws.add(st * MONORTM_NCONT), w_OL = ws.add(st);
    if (int rc = jac_ws_reserve(c, ws.size)) return rc;
    char *wb = static_cast<char *>(c->jac_ws);
    const ModmOut mo{.O = O, .O_BY_MOL = wb + w_OM, .OC = wb + w_OC, .O_CLW = wb + w_OL};
    if (int rc = modm_dev_impl(c, atm, false, mo, s)) return rc;   // (ixsect = 0: the entries have no cross-section arguments)
    return rtm_obs_dev_impl(c, atm, sfc, scan, O, obs, vcen, Y, out_kind, s);
}

}  // namespace

extern "C" {

int monortm_hip_obs_create(void *ctx, int npath, int nwn, int nview, int nchan, const int *view_start, const double *wpath, const int *chan,
                           const double *wchan, int *handle) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!handle) { c->err = "null handle pointer"; return MONORTM_EARG; }
    *handle = 0;
    if (int rc = obs_check(c, npath, nwn, nview, nchan, view_start, wpath, chan, wchan)) return rc;
    int slot = -1;
    for (int i = 0; i < Ctx::kMaxObs && slot < 0; i++)
        if (!c->obs[i].handle) slot = i;
    if (slot < 0) { c->err = "all " + std::to_string(Ctx::kMaxObs) + " measurement operators of the context are in use: destroy one"; return MONORTM_EARG; }
    DeviceGuard guard;
    Ctx::Obs ob;
    ob.npath = npath; ob.nwn = nwn; ob.nview = nview; ob.nchan = nchan;
    if (!c->shards.empty()) {
        for (Ctx *sh : c->shards) {
            int hs = 0;
            const int rc = monortm_hip_obs_create(sh, npath, nwn, nview, nchan, view_start, wpath, chan, wchan, &hs);
            if (rc) {
                c->err = "device " + std::to_string(sh->device) + ": " + sh->err;
                for (size_t g = 0; g < ob.shard.size(); g++) monortm_hip_obs_destroy(c->shards[g], ob.shard[g]);
                return rc;
            }
            ob.shard.push_back(hs);
        }
    } else if (int rc = obs_upload(c, ob, view_start, wpath, chan, wchan)) {
        return rc;
    }
    // a handle is never given out twice in a process: a stale one and one of another context are both told apart
    static std::atomic<unsigned> seq{0};
    const unsigned q = seq.fetch_add(1) % 0x3ffffffu + 1;
    ob.handle = (int)(q * Ctx::kMaxObs + slot);
    c->obs[slot] = ob;
    *handle = ob.handle;
    return MONORTM_OK;
}

int monortm_hip_obs_destroy(void *ctx, int handle) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    Ctx::Obs *ob = obs_find(c, handle);
    if (!ob) return obs_bad_handle(c);
    DeviceGuard guard;
    for (size_t g = 0; g < ob->shard.size(); g++) monortm_hip_obs_destroy(c->shards[g], ob->shard[g]);
    if (ob->dev) {
        hipSetDevice(c->device);
        hipDeviceSynchronize();   // no launch that reads the tables is still in flight
        hipFree(ob->dev);
    }
    *ob = Ctx::Obs();
    return MONORTM_OK;
}

// ---- Jacobians ----------------------------------------------------------------------------------
int monortm_hip_rtm_jac_dev(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt, int quantity,
                            const void *T, const void *TZ, const void *O, const void *tmpsfc, const void *emiss, const void *reflc,
                            void *RAD, void *TB, void *K_O, void *K_T, void *K_TZ, void *K_SFC, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacOut out{.RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_O = K_O, .K_SFC = K_SFC};
    return rtm_jac_dev_impl(c, atm, sfc, O, out, (hipStream_t)stream);
}

int monortm_hip_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                                double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const void *XAMNT, const int *irt,
                                const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac,
                                const int *jac_mol, void *O, void *RAD, void *TB, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O,
                                void *K_SFC, const double *wn_ends, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT, .wn_ends = wn_ends};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const JacOut out{.O = O, .RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_O = K_O, .K_SFC = K_SFC};
    return jac_full(c, JAC_PLAIN, atm, sfc, jq, ScanIn(), 0, out, (hipStream_t)stream);
}

int monortm_hip_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                             const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                             double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc,
                             const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, void *O, void *RAD,
                             void *TB, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O, void *K_SFC, const double *wn_ends,
                             void *stream) {
    return monortm_hip_jacobian_xs_dev(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                                       ibrd, 0, nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, O, RAD, TB, K_T, K_TZ, K_W, K_CLW,
                                       K_O, K_SFC, wn_ends, stream);
}

int monortm_hip_rtm_jac(void *ctx, int nprof, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt, int quantity,
                        const void *T, const void *TZ, const void *O, const void *tmpsfc, const void *emiss, const void *reflc, void *RAD,
                        void *TB, void *K_O, void *K_T, void *K_TZ, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    if (any_null({wn, nlay, irt, T, TZ, O, tmpsfc, emiss, reflc, RAD, TB, K_O, K_T, K_TZ, K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    DeviceGuard guard;
    if (int rc = jac_check_args(c, atm, quantity)) return rc;
    const size_t d = (size_t)c->real_kind, l = (size_t)nlay_max * d, v = (size_t)nwn * d, w = l * nwn;
    HostCall hc(8);
    const HostIn in = declare_inputs(hc, c, atm, sfc, ScanIn(), O);
    const int o_rad = hc.out(RAD, v), o_tb = hc.out(TB, v), o_ko = hc.out(K_O, w), o_kt = hc.out(K_T, w), o_ktz = hc.out(K_TZ, (l + d) * nwn),
              o_ks = hc.out(K_SFC, 3 * v);
    return hc.run(c, nprof, [&](Ctx *s, int, int n, char *const *dv) {
        const Share sh(in, dv, n, atm, sfc, ScanIn());
        const JacOut out{.RAD = dv[o_rad], .TB = dv[o_tb], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_O = dv[o_ko], .K_SFC = dv[o_ks]};
        return rtm_jac_dev_impl(s, sh.atm, sh.sfc, sh.O, out, s->hs);
    });
}

int monortm_hip_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                            const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                            double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const void *XAMNT, const int *irt, const void *TZ,
                            const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, void *O,
                            void *RAD, void *TB, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const JacOut out{.O = O, .RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_O = K_O, .K_SFC = K_SFC};
    if (int rc = need_real8(c, kJacEntry[JAC_PLAIN])) return rc;
    if (jac_full_null(JAC_PLAIN, atm, sfc, ScanIn(), out)) { c->err = "null array argument"; return MONORTM_EARG; }
    DeviceGuard guard;
    if (int rc = jac_check_args(c, atm, quantity)) return rc;
    if (int rc = jac_check_mol(c, atm, jq, K_W)) return rc;
    const size_t d = 8, l = (size_t)nlay_max * d, v = (size_t)nwn * d, w = l * nwn;
    HostCall hc(8);
    hc.flag = true;
    const HostIn in = declare_inputs(hc, c, atm, sfc, ScanIn(), nullptr);
    const int o_O = hc.out(O, w), o_rad = hc.out(RAD, v), o_tb = hc.out(TB, v), o_kt = hc.out(K_T, w), o_ktz = hc.out(K_TZ, (l + d) * nwn),
              o_kw = hc.out(njac ? K_W : nullptr, w * njac), o_kc = hc.out(K_CLW, w), o_ko = hc.out(K_O, w), o_ks = hc.out(K_SFC, 3 * v);
    // every share's states are checked on its own device's context, before anything of it is staged
    auto pre = [&](Ctx *s, int p0, int n) -> int {
        if (nmol < 1) { s->err = "bad nmol"; return MONORTM_EARG; }
        AtmIn share = atm;
        share.nprof = n; share.nlay = nlay + p0; share.T = hc.host(in.T, p0);
        return jac_check_states(s, share);
    };
    return hc.run(c, nprof, pre, [&](Ctx *s, int, int n, char *const *dv) {
        const Share sh(in, dv, n, atm, sfc, ScanIn());
        const JacOut od{.O = dv[o_O], .RAD = dv[o_rad], .TB = dv[o_tb], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_W = dv[o_kw], .K_CLW = dv[o_kc],
                        .K_O = dv[o_ko], .K_SFC = dv[o_ks]};
        return jac_full(s, JAC_PLAIN, sh.atm, sh.sfc, jq, sh.scan, 0, od, s->hs);
    });
}

int monortm_hip_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                         const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                         double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc,
                         const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, void *O, void *RAD, void *TB,
                         void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O, void *K_SFC) {
    return monortm_hip_jacobian_xs(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res, ibrd, 0,
                                   nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, O, RAD, TB, K_T, K_TZ, K_W, K_CLW, K_O, K_SFC);
}

// ---- Jacobians of path scans ----------------------------------------------------------------------
int monortm_hip_rtm_scan_jac_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                                 int quantity, const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc,
                                 int sfc_per_path, const void *emiss, const void *reflc, void *RAD, void *TB, void *K_O, void *K_PATH,
                                 void *K_T, void *K_TZ, void *K_SFC, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_O = K_O, .K_PATH = K_PATH, .K_SFC = K_SFC};
    return rtm_scan_jac_dev_impl(c, atm, sfc, scan, O, out, (hipStream_t)stream);
}

int monortm_hip_scan_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                     const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL,
                                     const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd, int ixsect,
                                     const void *XAMNT, const int *irt, const void *TZ, const void *tmpsfc, const void *emiss,
                                     const void *reflc, int quantity, int njac, const int *jac_mol, int npath, const void *path,
                                     int sfc_per_path, void *O, void *RAD, void *TB, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O,
                                     void *K_PATH, void *K_SFC, const double *wn_ends, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT, .wn_ends = wn_ends};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.O = O, .RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_O = K_O, .K_PATH = K_PATH,
                     .K_SFC = K_SFC};
    return jac_full(c, JAC_SCAN, atm, sfc, jq, scan, 0, out, (hipStream_t)stream);
}

int monortm_hip_scan_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                  const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL,
                                  const double *cntnm_fac, double sclcpl, double sclhw, double y0res, int ibrd, const int *irt,
                                  const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac,
                                  const int *jac_mol, int npath, const void *path, int sfc_per_path, void *O, void *RAD, void *TB, void *K_T,
                                  void *K_TZ, void *K_W, void *K_CLW, void *K_O, void *K_PATH, void *K_SFC, const double *wn_ends,
                                  void *stream) {
    return monortm_hip_scan_jacobian_xs_dev(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                                            ibrd, 0, nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, npath, path, sfc_per_path, O,
                                            RAD, TB, K_T, K_TZ, K_W, K_CLW, K_O, K_PATH, K_SFC, wn_ends, stream);
}

int monortm_hip_rtm_scan_jac(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                             int quantity, const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc,
                             int sfc_per_path, const void *emiss, const void *reflc, void *RAD, void *TB, void *K_O, void *K_PATH, void *K_T,
                             void *K_TZ, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, irt, T, TZ, O, path, tmpsfc, emiss, reflc, RAD, TB, K_T, K_TZ, K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rc = check_quantity(c, quantity)) return rc;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    // the whole call's nlay and factors before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    const size_t d = (size_t)c->real_kind, l = (size_t)nlay_max * d, vo = (size_t)nwn * npath * d, wo = l * nwn * npath;
    HostCall hc(8);
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, O);
    const int o_rad = hc.out(RAD, vo), o_tb = hc.out(TB, vo), o_ko = hc.out(K_O, wo), o_kp = hc.out(K_PATH, wo), o_kt = hc.out(K_T, wo),
              o_ktz = hc.out(K_TZ, (l + d) * nwn * npath), o_ks = hc.out(K_SFC, 3 * vo);
    return hc.run(c, nprof, [&](Ctx *s, int, int n, char *const *dv) {
        const Share sh(in, dv, n, atm, sfc, scan);
        const JacOut out{.RAD = dv[o_rad], .TB = dv[o_tb], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_O = dv[o_ko], .K_PATH = dv[o_kp],
                         .K_SFC = dv[o_ks]};
        return rtm_scan_jac_dev_impl(s, sh.atm, sh.sfc, sh.scan, sh.O, out, s->hs);
    });
}

int monortm_hip_scan_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                 const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                                 double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const void *XAMNT, const int *irt,
                                 const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac,
                                 const int *jac_mol, int npath, const void *path, int sfc_per_path, void *O, void *RAD, void *TB, void *K_T,
                                 void *K_TZ, void *K_W, void *K_CLW, void *K_O, void *K_PATH, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.O = O, .RAD = RAD, .TB = TB, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_O = K_O, .K_PATH = K_PATH,
                     .K_SFC = K_SFC};
    if (int rc = need_real8(c, kJacEntry[JAC_SCAN])) return rc;
    if (jac_full_null(JAC_SCAN, atm, sfc, scan, out)) { c->err = "null array argument"; return MONORTM_EARG; }
    DeviceGuard guard;
    // the whole call is checked before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (int rc = jac_check_args(c, atm, quantity)) return rc;
    if (int rc = jac_check_mol(c, atm, jq, K_W)) return rc;
    if (nmol < 1) { c->err = "bad nmol"; return MONORTM_EARG; }
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    if (int rc = jac_check_states(c, atm)) return rc;
    const size_t d = 8, l = (size_t)nlay_max * d, w = l * nwn, vo = (size_t)nwn * npath * d, wo = w * npath;
    HostCall hc(8);
    hc.flag = true;
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, nullptr);
    const int o_O = hc.out(O, w), o_rad = hc.out(RAD, vo), o_tb = hc.out(TB, vo), o_kt = hc.out(K_T, wo), o_ktz = hc.out(K_TZ, (l + d) * nwn * npath),
              o_kw = hc.out(njac ? K_W : nullptr, wo * njac), o_kc = hc.out(K_CLW, wo), o_ko = hc.out(K_O, wo), o_kp = hc.out(K_PATH, wo),
              o_ks = hc.out(K_SFC, 3 * vo);
    return hc.run(c, nprof, [&](Ctx *s, int, int n, char *const *dv) {
        const Share sh(in, dv, n, atm, sfc, scan);
        const JacOut od{.O = dv[o_O], .RAD = dv[o_rad], .TB = dv[o_tb], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_W = dv[o_kw], .K_CLW = dv[o_kc],
                        .K_O = dv[o_ko], .K_PATH = dv[o_kp], .K_SFC = dv[o_ks]};
        return jac_full(s, JAC_SCAN, sh.atm, sh.sfc, jq, sh.scan, 0, od, s->hs);
    });
}

int monortm_hip_scan_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                              const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                              double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc,
                              const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, int npath, const void *path,
                              int sfc_per_path, void *O, void *RAD, void *TB, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_O,
                              void *K_PATH, void *K_SFC) {
    return monortm_hip_scan_jacobian_xs(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                                        ibrd, 0, nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, npath, path, sfc_per_path, O, RAD,
                                        TB, K_T, K_TZ, K_W, K_CLW, K_O, K_PATH, K_SFC);
}

// ---- channel- and beam-averaged Jacobians of path scans ---------------------------------------------
int monortm_hip_rtm_obs_jac_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                                int quantity, const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc,
                                int sfc_per_path, const void *emiss, const void *reflc, int obs, void *Y, void *K_T, void *K_TZ, void *K_SFC,
                                void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.Y = Y, .K_T = K_T, .K_TZ = K_TZ, .K_SFC = K_SFC};
    return rtm_obs_jac_dev_impl(c, atm, sfc, scan, O, obs, out, c->real_kind, (hipStream_t)stream);
}

int monortm_hip_obs_jacobian_xs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                    const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                                    double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const void *XAMNT, const int *irt,
                                    const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac,
                                    const int *jac_mol, int npath, const void *path, int sfc_per_path, int obs, void *O, void *Y, void *K_T,
                                    void *K_TZ, void *K_W, void *K_CLW, void *K_SFC, const double *wn_ends, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT, .wn_ends = wn_ends};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.O = O, .Y = Y, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_SFC = K_SFC};
    return jac_full(c, JAC_OBS, atm, sfc, jq, scan, obs, out, (hipStream_t)stream);
}

int monortm_hip_obs_jacobian_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                 const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                                 double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc,
                                 const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, int npath, const void *path,
                                 int sfc_per_path, int obs, void *O, void *Y, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_SFC,
                                 const double *wn_ends, void *stream) {
    return monortm_hip_obs_jacobian_xs_dev(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                                           ibrd, 0, nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, npath, path, sfc_per_path, obs,
                                           O, Y, K_T, K_TZ, K_W, K_CLW, K_SFC, wn_ends, stream);
}

int monortm_hip_rtm_obs_jac(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                            int quantity, const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc, int sfc_per_path,
                            const void *emiss, const void *reflc, int obs, void *Y, void *K_T, void *K_TZ, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, irt, T, TZ, O, path, tmpsfc, emiss, reflc, Y, K_T, K_TZ, K_SFC})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    if (int rc = check_quantity(c, quantity)) return rc;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, npath, nwn, &ob)) return rc;
    // the whole call's nlay and factors before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    const size_t y = (size_t)ob->nview * ob->nchan;   // measurements of a profile
    HostCall hc(8);
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, O);
    // the kernel accumulates into double outputs (out_kind 8) whatever the context's REAL kind: rounded once, when they are unpacked
    const int o_y = hc.out_widened(Y, y), o_kt = hc.out_widened(K_T, y * nlay_max), o_ktz = hc.out_widened(K_TZ, y * (nlay_max + 1)),
              o_ks = hc.out_widened(K_SFC, 3 * y);
    return hc.run(c, nprof, [&](Ctx *s, int g, int n, char *const *dv) {   // (every shard holds the operator under a handle of its own)
        const Share sh(in, dv, n, atm, sfc, scan);
        const JacOut out{.Y = dv[o_y], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_SFC = dv[o_ks]};
        return rtm_obs_jac_dev_impl(s, sh.atm, sh.sfc, sh.scan, sh.O, g < 0 ? obs : ob->shard[g], out, 8, s->hs);
    });
}

int monortm_hip_obs_jacobian_xs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                                const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                                double sclcpl, double sclhw, double y0res, int ibrd, int ixsect, const void *XAMNT, const int *irt,
                                const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc, int quantity, int njac,
                                const int *jac_mol, int npath, const void *path, int sfc_per_path, int obs, void *O, void *Y, void *K_T,
                                void *K_TZ, void *K_W, void *K_CLW, void *K_SFC) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .ixsect = ixsect, .XAMNT = XAMNT};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const JacReq jq{.njac = njac, .jac_mol = jac_mol};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    const JacOut out{.O = O, .Y = Y, .K_T = K_T, .K_TZ = K_TZ, .K_W = K_W, .K_CLW = K_CLW, .K_SFC = K_SFC};
    if (int rc = need_real8(c, kJacEntry[JAC_OBS])) return rc;
    if (jac_full_null(JAC_OBS, atm, sfc, scan, out)) { c->err = "null array argument"; return MONORTM_EARG; }
    DeviceGuard guard;
    // the whole call is checked before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (int rc = jac_check_args(c, atm, quantity)) return rc;
    if (int rc = jac_check_mol(c, atm, jq, K_W)) return rc;
    if (nmol < 1) { c->err = "bad nmol"; return MONORTM_EARG; }
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, npath, nwn, &ob)) return rc;
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    if (int rc = jac_check_states(c, atm)) return rc;
    const size_t d = 8, l = (size_t)nlay_max * d;
    const size_t y = (size_t)ob->nview * ob->nchan * d, yk = y * nlay_max;   // bytes of a profile's measurements, of their layer derivatives
    HostCall hc(8);
    hc.flag = true;
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, nullptr);
    const int o_O = hc.out(O, l * nwn), o_y = hc.out(Y, y), o_kt = hc.out(K_T, yk), o_ktz = hc.out(K_TZ, yk + y),
              o_kw = hc.out(njac ? K_W : nullptr, yk * njac), o_kc = hc.out(K_CLW, yk), o_ks = hc.out(K_SFC, 3 * y);
    return hc.run(c, nprof, [&](Ctx *s, int g, int n, char *const *dv) {   // (every shard holds the operator under a handle of its own)
        const Share sh(in, dv, n, atm, sfc, scan);
        const JacOut od{.O = dv[o_O], .Y = dv[o_y], .K_T = dv[o_kt], .K_TZ = dv[o_ktz], .K_W = dv[o_kw], .K_CLW = dv[o_kc], .K_SFC = dv[o_ks]};
        return jac_full(s, JAC_OBS, sh.atm, sh.sfc, jq, sh.scan, g < 0 ? obs : ob->shard[g], od, s->hs);
    });
}

int monortm_hip_obs_jacobian(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol,
                             const void *P, const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac,
                             double sclcpl, double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc,
                             const void *emiss, const void *reflc, int quantity, int njac, const int *jac_mol, int npath, const void *path,
                             int sfc_per_path, int obs, void *O, void *Y, void *K_T, void *K_TZ, void *K_W, void *K_CLW, void *K_SFC) {
    return monortm_hip_obs_jacobian_xs(ctx, nprof, nwn, wn, dvset, nlay, nlay_max, nmol, P, T, CLW, WKL, WBRODL, cntnm_fac, sclcpl, sclhw, y0res,
                                       ibrd, 0, nullptr, irt, TZ, tmpsfc, emiss, reflc, quantity, njac, jac_mol, npath, path, sfc_per_path, obs, O, Y,
                                       K_T, K_TZ, K_W, K_CLW, K_SFC);
}

// ---- the forward measurement operator -----------------------------------------------------------------------
int monortm_hip_rtm_obs_dev(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt,
                            int quantity, const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc, int sfc_per_path,
                            const void *emiss, const void *reflc, int obs, const double *vcen, void *Y, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    return rtm_obs_dev_impl(c, atm, sfc, scan, O, obs, vcen, Y, c->real_kind, (hipStream_t)stream);
}

int monortm_hip_obs_dev(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol, const void *P,
                        const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac, double sclcpl,
                        double sclhw, double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc, const void *emiss,
                        const void *reflc, int quantity, int npath, const void *path, int sfc_per_path, int obs, const double *vcen, void *O,
                        void *Y, const double *wn_ends, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd, .wn_ends = wn_ends};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    return obs_dev_impl(c, atm, sfc, scan, obs, vcen, O, Y, c->real_kind, (hipStream_t)stream);
}

int monortm_hip_rtm_obs(void *ctx, int nprof, int npath, int nwn, const double *wn, const int *nlay, int nlay_max, const int *irt, int quantity,
                        const void *T, const void *TZ, const void *O, const void *path, const void *tmpsfc, int sfc_per_path, const void *emiss,
                        const void *reflc, int obs, const double *vcen, void *Y) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .nlay = nlay, .nlay_max = nlay_max, .T = T};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, irt, T, TZ, O, path, tmpsfc, emiss, reflc, Y})) { c->err = "null array argument"; return MONORTM_EARG; }
    if (int rc = obs_check_quantity(c, quantity)) return rc;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, npath, nwn, &ob)) return rc;
    if (int rc = obs_check_vcen(c, quantity, vcen, ob->nchan)) return rc;
    // the whole call's nlay and factors before the first device is touched: a refusal launches nothing anywhere
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    HostCall hc(4);   // (the scan slots: lastO, which points into the MODM slots, stays valid)
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, O);
    const int i_vc = hc.in_shared(quantity == 2 ? vcen : nullptr, ob->nchan * sizeof(double));
    // the kernel accumulates into a double Y (out_kind 8) whatever the context's REAL kind: rounded once, when it is unpacked
    const int o_y = hc.out_widened(Y, (size_t)ob->nview * ob->nchan);
    return hc.run(c, nprof, [&](Ctx *s, int g, int n, char *const *dv) {   // (every shard holds the operator under a handle of its own)
        const Share sh(in, dv, n, atm, sfc, scan);
        return rtm_obs_dev_impl(s, sh.atm, sh.sfc, sh.scan, sh.O, g < 0 ? obs : ob->shard[g], (double *)dv[i_vc], dv[o_y], 8, s->hs);
    });
}

int monortm_hip_obs(void *ctx, int nprof, int nwn, const double *wn, double dvset, const int *nlay, int nlay_max, int nmol, const void *P,
                    const void *T, const void *CLW, const void *WKL, const void *WBRODL, const double *cntnm_fac, double sclcpl, double sclhw,
                    double y0res, int ibrd, const int *irt, const void *TZ, const void *tmpsfc, const void *emiss, const void *reflc,
                    int quantity, int npath, const void *path, int sfc_per_path, int obs, const double *vcen, void *O, void *Y) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const AtmIn atm{.nprof = nprof, .nwn = nwn, .wn = wn, .dvset = dvset, .nlay = nlay, .nlay_max = nlay_max, .nmol = nmol, .P = P, .T = T,
                    .CLW = CLW, .WKL = WKL, .WBRODL = WBRODL, .cntnm_fac = cntnm_fac, .sclcpl = sclcpl, .sclhw = sclhw, .y0res = y0res,
                    .ibrd = ibrd};
    const SfcIn sfc{.irt = irt, .TZ = TZ, .tmpsfc = tmpsfc, .emiss = emiss, .reflc = reflc, .quantity = quantity};
    const ScanIn scan{.npath = npath, .path = path, .sfc_per_path = sfc_per_path};
    if (any_null({wn, nlay, P, T, CLW, WKL, WBRODL, cntnm_fac, irt, TZ, tmpsfc, emiss, reflc, path, O, Y})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    DeviceGuard guard;
    // the whole call is checked before the first device is touched: a refusal launches nothing anywhere
    if (int rc = obs_check_quantity(c, quantity)) return rc;
    if (int rc = scan_check_args(c, atm, scan)) return rc;
    if (nmol < 7 || nmol > MXMOL) { c->err = "nmol must be 7..39 (LINES reads WK(1:7), modm.f90:313)"; return MONORTM_EARG; }
    Ctx::Obs *ob = nullptr;
    if (int rc = obs_for_call(c, obs, npath, nwn, &ob)) return rc;
    if (int rc = obs_check_vcen(c, quantity, vcen, ob->nchan)) return rc;
    if (int rc = scan_check_path(c, atm, scan)) return rc;
    if (int rc = check_ascending(c, atm)) return rc;
    HostCall hc(8);   // (the Jacobian slots: a call between a MODM and an RTM call leaves lastO alone)
    hc.flag = true;
    const HostIn in = declare_inputs(hc, c, atm, sfc, scan, nullptr);
    const int i_vc = hc.in_shared(quantity == 2 ? vcen : nullptr, ob->nchan * sizeof(double));
    const int o_O = hc.out(O, (size_t)nlay_max * c->real_kind * nwn), o_y = hc.out_widened(Y, (size_t)ob->nview * ob->nchan);
    return hc.run(c, nprof, [&](Ctx *s, int g, int n, char *const *dv) {   // (every shard holds the operator under a handle of its own)
        const Share sh(in, dv, n, atm, sfc, scan);
        return obs_dev_impl(s, sh.atm, sh.sfc, sh.scan, g < 0 ? obs : ob->shard[g], (double *)dv[i_vc], dv[o_O], dv[o_y], 8, s->hs);
    });
}

// ---- the optimal-estimation step -----------------------------------------------------------------------
}  // extern "C"

namespace {
constexpr int kOeMaxMeas = 128, kOeMaxState = 2048;
// rows of the K array of each state kind: K_T, K_TZ, K_W, K_CLW, K_SFC
void oe_rows(int nlay_max, int njac, long long rows[5]) {
    rows[0] = nlay_max; rows[1] = (long long)nlay_max + 1; rows[2] = (long long)nlay_max * njac; rows[3] = nlay_max; rows[4] = 3;
}
// everything a host can check of a call, before anything is launched (the host entry: before anything is staged on any device)
int oe_check(Ctx *c, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind, const int *state_row,
             const void *const K[5], int sa_per_profile, int se_per_profile) {
    if (c->real_kind != 8) {
        c->err = "monortm_hip_oe_step needs a real_kind = 8 context (it reads the K arrays of the full Jacobians)";
        return MONORTM_EUNSUPPORTED;
    }
    if (nprof < 1 || nview < 1 || nchan < 1 || nlay_max < 1 || nlay_max > 603 || njac < 0 || njac > MXMOL) { c->err = "bad nprof/nview/nchan/nlay_max/njac"; return MONORTM_EARG; }
    if ((long long)nview * nchan > kOeMaxMeas) { c->err = "nmeas = nview x nchan outside 1.." + std::to_string(kOeMaxMeas); return MONORTM_EARG; }
    if (nstate < 1 || nstate > kOeMaxState) { c->err = "nstate outside 1.." + std::to_string(kOeMaxState); return MONORTM_EARG; }
    if ((sa_per_profile != 0 && sa_per_profile != 1) || (se_per_profile != 0 && se_per_profile != 1)) { c->err = "sa_per_profile / se_per_profile must be 0 or 1"; return MONORTM_EARG; }
    if (!state_kind || !state_row) { c->err = "null state map"; return MONORTM_EARG; }
    long long rows[5];
    oe_rows(nlay_max, njac, rows);
    static const char *const names[5] = {"K_T", "K_TZ", "K_W", "K_CLW", "K_SFC"};
    for (int s = 0; s < nstate; s++) {
        const int k = state_kind[s];
        if (k < 0 || k > 4) { c->err = "state " + std::to_string(s) + ": kind " + std::to_string(k) + " outside 0..4"; return MONORTM_EARG; }
        if (state_row[s] < 0 || state_row[s] >= rows[k]) {
            c->err = "state " + std::to_string(s) + ": row " + std::to_string(state_row[s]) + " outside the " + std::to_string(rows[k]) + " rows of " + names[k];
            return MONORTM_EARG;
        }
        if (!K[k]) { c->err = "state " + std::to_string(s) + " reads " + names[k] + ", which is null"; return MONORTM_EARG; }
    }
    return MONORTM_OK;
}
int oe_check_kind(Ctx *c, int se_kind) {
    if (se_kind != 0 && se_kind != 1) { c->err = "se_kind must be 0 ([nmeas] variances) or 1 ([nmeas][nmeas], lower triangle)"; return MONORTM_EARG; }
    return MONORTM_OK;
}

// the device entries: se is [nmeas] (se_kind 0) or Se [nmeas][nmeas] (1); gain_t, avk, post_cov, dofs null for monortm_hip_oe_step_dev;
// cdual, c_new, cost null for it and for monortm_hip_oe_step_full_dev
int oe_step_dev_impl(Ctx *c, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind, const int *state_row,
                     const void *const K[5], const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile,
                     const void *se, int se_kind, int se_per_profile, const void *gamma, void *x_new, void *post_var, void *avk_diag,
                     void *chi2, int *status, void *gain_t, void *avk, void *post_cov, void *dofs, const void *cdual, void *c_new, void *cost,
                     void *stream) {
    if (!c->shards.empty()) return multi_only_host(c);
    if (int rc = oe_check(c, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, sa_per_profile, se_per_profile)) return rc;
    if (int rc = oe_check_kind(c, se_kind)) return rc;
    if (!Y || !y_obs || !x || !xa || !Sa || !se || !x_new || !status) { c->err = "null array argument"; return MONORTM_EARG; }
    if (cdual && cdual == c_new) { c->err = "c_new must not be c itself (the cost reads c behind the stores to c_new)"; return MONORTM_EARG; }
    if (int rcd = check_device(c)) return rcd;
    hipStream_t s = (hipStream_t)stream;
    const int nmeas = nview * nchan;
    // the state map: kinds, then rows x nchan.  It travels only when it differs from the one the device holds, and then behind
    // whatever still reads the old one (that wait cannot be captured: the warm call of a capture has brought the map over)
    std::vector<int> map(2 * (size_t)nstate);
    for (int i = 0; i < nstate; i++) { map[i] = state_kind[i]; map[nstate + i] = state_row[i] * nchan; }
    if (map != c->oe_map_host) {
        HIPCHK(c, hipStreamSynchronize(s));
        c->oe_map_host.clear();
        HIPCHK(c, grow(&c->oe_map, &c->oe_map_ints, map.size(), sizeof(int)));
        HIPCHK(c, hipMemcpy(c->oe_map, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
        c->oe_map_host = map;
    }
    HIPCHK(c, grow(&c->oe_ws, &c->oe_ws_elems, (size_t)nprof * 2 * nmeas * nstate, sizeof(double)));
    if (dofs && !avk_diag) {   // the kernel sums the diagonal it stored
        HIPCHK(c, grow(&c->oe_diag, &c->oe_diag_elems, (size_t)nprof * nstate, sizeof(double)));
        avk_diag = c->oe_diag;
    }
    OeArgs a{};
    a.nprof = nprof; a.nview = nview; a.nchan = nchan; a.nmeas = nmeas; a.nstate = nstate;
    a.sa_per_profile = sa_per_profile; a.se_per_profile = se_per_profile;
    long long rows[5];
    oe_rows(nlay_max, njac, rows);
    for (int k = 0; k < 5; k++) {
        a.K[k] = static_cast<const double *>(K[k]);
        a.vstride[k] = (int)(rows[k] * nchan);
        a.kstride[k] = (size_t)nview * rows[k] * nchan;
    }
    a.map = static_cast<const int *>(c->oe_map);
    a.Y = (const double *)Y; a.y_obs = (const double *)y_obs; a.x = (const double *)x; a.xa = (const double *)xa; a.Sa = (const double *)Sa;
    a.se = (const double *)se; a.gamma = (const double *)gamma;
    a.x_new = (double *)x_new; a.post_var = (double *)post_var; a.avk_diag = (double *)avk_diag; a.chi2 = (double *)chi2; a.status = status;
    a.ws = static_cast<double *>(c->oe_ws);
    a.se_kind = se_kind; a.gain_t = (double *)gain_t; a.dofs = (double *)dofs;
    a.c = (const double *)cdual; a.c_new = (double *)c_new; a.cost = (double *)cost;
    HIPCHK(c, launch_oe_step(a, s));
    OeCovArgs v{};
    v.nprof = nprof; v.nmeas = nmeas; v.nstate = nstate; v.sa_per_profile = sa_per_profile;
    v.ws = a.ws; v.Sa = a.Sa; v.gamma = a.gamma; v.status = status;
    v.avk = (double *)avk; v.post_cov = (double *)post_cov;
    HIPCHK(c, launch_oe_cov(v, s));   // (no launch without a matrix)
    return MONORTM_OK;
}
}  // namespace

extern "C" {

int monortm_hip_oe_step_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                            const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW, const void *K_SFC,
                            const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile, const void *se,
                            int se_per_profile, const void *gamma, void *x_new, void *post_var, void *avk_diag, void *chi2, int *status,
                            void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    return oe_step_dev_impl(c, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, Y, y_obs, x, xa, Sa, sa_per_profile, se, 0,
                            se_per_profile, gamma, x_new, post_var, avk_diag, chi2, status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            stream);
}

int monortm_hip_oe_step_full_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                                 const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW,
                                 const void *K_SFC, const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa,
                                 int sa_per_profile, const void *Se, int se_kind, int se_per_profile, const void *gamma, void *x_new,
                                 void *post_var, void *avk_diag, void *chi2, int *status, void *gain_t, void *avk, void *post_cov, void *dofs,
                                 void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    return oe_step_dev_impl(c, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, Y, y_obs, x, xa, Sa, sa_per_profile, Se,
                            se_kind, se_per_profile, gamma, x_new, post_var, avk_diag, chi2, status, gain_t, avk, post_cov, dofs, nullptr, nullptr, nullptr,
                            stream);
}

int monortm_hip_oe_step(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                        const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW, const void *K_SFC,
                        const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile, const void *se,
                        int se_per_profile, const void *gamma, void *x_new, void *post_var, void *avk_diag, void *chi2, int *status) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    if (int rc = oe_check(c, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, sa_per_profile, se_per_profile)) return rc;
    if (!Y || !y_obs || !x || !xa || !Sa || !se || !x_new || !status) { c->err = "null array argument"; return MONORTM_EARG; }
    long long rows[5];
    oe_rows(nlay_max, njac, rows);
    const size_t d = 8, y = (size_t)nview * nchan * d, n = (size_t)nstate * d;
    HostCall hc(8);
    int i_K[5];
    for (int k = 0; k < 5; k++) i_K[k] = hc.in(K[k], y * rows[k]);
    const int i_Y = hc.in(Y, y), i_yo = hc.in(y_obs, y), i_x = hc.in(x, n), i_xa = hc.in(xa, n),
              i_Sa = sa_per_profile ? hc.in(Sa, n * nstate) : hc.in_shared(Sa, n * nstate), i_se = se_per_profile ? hc.in(se, y) : hc.in_shared(se, y),
              i_g = hc.in(gamma, d);
    const int o_x = hc.out(x_new, n), o_pv = hc.out(post_var, n), o_av = hc.out(avk_diag, n), o_c2 = hc.out(chi2, d), o_st = hc.out(status, sizeof(int));
    return hc.run(c, nprof, [&](Ctx *s, int, int np, char *const *dv) {
        return monortm_hip_oe_step_dev(s, np, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, dv[i_K[0]], dv[i_K[1]], dv[i_K[2]],
                                       dv[i_K[3]], dv[i_K[4]], dv[i_Y], dv[i_yo], dv[i_x], dv[i_xa], dv[i_Sa], sa_per_profile, dv[i_se],
                                       se_per_profile, dv[i_g], dv[o_x], dv[o_pv], dv[o_av], dv[o_c2], (int *)dv[o_st], s->hs);
    });
}

int monortm_hip_oe_step_full(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                             const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW, const void *K_SFC,
                             const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile,
                             const void *Se, int se_kind, int se_per_profile, const void *gamma, void *x_new, void *post_var, void *avk_diag,
                             void *chi2, int *status, void *gain_t, void *avk, void *post_cov, void *dofs) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    DeviceGuard guard;
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    if (int rc = oe_check(c, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, sa_per_profile, se_per_profile)) return rc;
    if (int rc = oe_check_kind(c, se_kind)) return rc;
    if (!Y || !y_obs || !x || !xa || !Sa || !Se || !x_new || !status) { c->err = "null array argument"; return MONORTM_EARG; }
    long long rows[5];
    oe_rows(nlay_max, njac, rows);
    const size_t d = 8, m = (size_t)nview * nchan, y = m * d, n = (size_t)nstate * d, e = se_kind ? y * m : y;
    HostCall hc(8);
    int i_K[5];
    for (int k = 0; k < 5; k++) i_K[k] = hc.in(K[k], y * rows[k]);
    const int i_Y = hc.in(Y, y), i_yo = hc.in(y_obs, y), i_x = hc.in(x, n), i_xa = hc.in(xa, n),
              i_Sa = sa_per_profile ? hc.in(Sa, n * nstate) : hc.in_shared(Sa, n * nstate), i_se = se_per_profile ? hc.in(Se, e) : hc.in_shared(Se, e),
              i_g = hc.in(gamma, d);
    const int o_x = hc.out(x_new, n), o_pv = hc.out(post_var, n), o_av = hc.out(avk_diag, n), o_c2 = hc.out(chi2, d), o_st = hc.out(status, sizeof(int)),
              o_gn = hc.out(gain_t, m * n), o_ak = hc.out(avk, n * nstate), o_pc = hc.out(post_cov, n * nstate), o_df = hc.out(dofs, d);
    return hc.run(c, nprof, [&](Ctx *s, int, int np, char *const *dv) {
        return monortm_hip_oe_step_full_dev(s, np, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, dv[i_K[0]], dv[i_K[1]],
                                            dv[i_K[2]], dv[i_K[3]], dv[i_K[4]], dv[i_Y], dv[i_yo], dv[i_x], dv[i_xa], dv[i_Sa], sa_per_profile,
                                            dv[i_se], se_kind, se_per_profile, dv[i_g], dv[o_x], dv[o_pv], dv[o_av], dv[o_c2], (int *)dv[o_st],
                                            dv[o_gn], dv[o_ak], dv[o_pc], dv[o_df], s->hs);
    });
}

// ---- the adaptive retrieval loop -------------------------------------------------------------------------
int monortm_hip_oe_step_lm_dev(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                               const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW, const void *K_SFC,
                               const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile,
                               const void *Se, int se_kind, int se_per_profile, const void *gamma, void *x_new, void *post_var,
                               void *avk_diag, void *chi2, int *status, void *gain_t, void *avk, void *post_cov, void *dofs, const void *c,
                               void *c_new, void *cost, void *stream) {
    Ctx *cx = static_cast<Ctx *>(ctx);
    if (!cx) return null_ctx();
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    return oe_step_dev_impl(cx, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, Y, y_obs, x, xa, Sa, sa_per_profile, Se,
                            se_kind, se_per_profile, gamma, x_new, post_var, avk_diag, chi2, status, gain_t, avk, post_cov, dofs, c, c_new, cost,
                            stream);
}

int monortm_hip_oe_step_lm(void *ctx, int nprof, int nview, int nchan, int nlay_max, int njac, int nstate, const int *state_kind,
                           const int *state_row, const void *K_T, const void *K_TZ, const void *K_W, const void *K_CLW, const void *K_SFC,
                           const void *Y, const void *y_obs, const void *x, const void *xa, const void *Sa, int sa_per_profile,
                           const void *Se, int se_kind, int se_per_profile, const void *gamma, void *x_new, void *post_var, void *avk_diag,
                           void *chi2, int *status, void *gain_t, void *avk, void *post_cov, void *dofs, const void *c, void *c_new,
                           void *cost) {
    Ctx *cx = static_cast<Ctx *>(ctx);
    if (!cx) return null_ctx();
    DeviceGuard guard;
    const void *const K[5] = {K_T, K_TZ, K_W, K_CLW, K_SFC};
    if (int rc = oe_check(cx, nprof, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, K, sa_per_profile, se_per_profile)) return rc;
    if (int rc = oe_check_kind(cx, se_kind)) return rc;
    if (!Y || !y_obs || !x || !xa || !Sa || !Se || !x_new || !status) { cx->err = "null array argument"; return MONORTM_EARG; }
    if (c && c == c_new) { cx->err = "c_new must not be c itself (the cost reads c behind the stores to c_new)"; return MONORTM_EARG; }
    long long rows[5];
    oe_rows(nlay_max, njac, rows);
    const size_t d = 8, m = (size_t)nview * nchan, y = m * d, n = (size_t)nstate * d, e = se_kind ? y * m : y;
    HostCall hc(8);
    int i_K[5];
    for (int k = 0; k < 5; k++) i_K[k] = hc.in(K[k], y * rows[k]);
    const int i_Y = hc.in(Y, y), i_yo = hc.in(y_obs, y), i_x = hc.in(x, n), i_xa = hc.in(xa, n),
              i_Sa = sa_per_profile ? hc.in(Sa, n * nstate) : hc.in_shared(Sa, n * nstate), i_se = se_per_profile ? hc.in(Se, e) : hc.in_shared(Se, e),
              i_g = hc.in(gamma, d), i_c = hc.in(c, n);
    const int o_x = hc.out(x_new, n), o_pv = hc.out(post_var, n), o_av = hc.out(avk_diag, n), o_c2 = hc.out(chi2, d), o_st = hc.out(status, sizeof(int)),
              o_gn = hc.out(gain_t, m * n), o_ak = hc.out(avk, n * nstate), o_pc = hc.out(post_cov, n * nstate), o_df = hc.out(dofs, d),
              o_cn = hc.out(c_new, n), o_J = hc.out(cost, d);
    return hc.run(cx, nprof, [&](Ctx *s, int, int np, char *const *dv) {
        return monortm_hip_oe_step_lm_dev(s, np, nview, nchan, nlay_max, njac, nstate, state_kind, state_row, dv[i_K[0]], dv[i_K[1]], dv[i_K[2]],
                                          dv[i_K[3]], dv[i_K[4]], dv[i_Y], dv[i_yo], dv[i_x], dv[i_xa], dv[i_Sa], sa_per_profile, dv[i_se],
                                          se_kind, se_per_profile, dv[i_g], dv[o_x], dv[o_pv], dv[o_av], dv[o_c2], (int *)dv[o_st], dv[o_gn],
                                          dv[o_ak], dv[o_pc], dv[o_df], dv[i_c], dv[o_cn], dv[o_J], s->hs);
    });
}

int monortm_hip_oe_scatter_dev(void *ctx, int nprof, int nstate, const int *map_kind, const int *map_index, const int *map_mol,
                               const void *x_src, const void *x_fallback, const int *done, const void *lo, const void *hi,
                               int box_per_profile, const int *nlay, int nlay_max, int nmol, void *T, long long t_stride, void *TZ,
                               long long tz_stride, void *WKL, long long wkl_stride, void *CLW, long long clw_stride, void *tmpsfc_a,
                               void *tmpsfc_b, int *trial_ok, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    if (c->real_kind != 8) { c->err = "monortm_hip_oe_scatter_dev needs a real_kind = 8 context"; return MONORTM_EUNSUPPORTED; }
    if (nprof < 1 || nlay_max < 1 || nlay_max > 603 || nmol < 0 || nmol > MXMOL) { c->err = "bad nprof/nlay_max/nmol"; return MONORTM_EARG; }
    if (nstate < 1 || nstate > kOeMaxState) { c->err = "nstate outside 1.." + std::to_string(kOeMaxState); return MONORTM_EARG; }
    if (box_per_profile != 0 && box_per_profile != 1) { c->err = "box_per_profile must be 0 or 1"; return MONORTM_EARG; }
    if (!map_kind || !map_index || !map_mol) { c->err = "null write map"; return MONORTM_EARG; }
    if (!x_src || !nlay) { c->err = "null array argument"; return MONORTM_EARG; }
    // every store the kernel can make, checked here: the array is given, the element lies inside a profile's stride, and no two
    // written columns share a target (the kernel's stores would race)
    const void *arr[4] = {T, TZ, WKL, CLW};
    const long long stride[4] = {t_stride, tz_stride, wkl_stride, clw_stride};
    static const char *const names[4] = {"T", "TZ", "WKL", "CLW"};
    std::vector<int> map(3 * (size_t)nstate);
    std::vector<long long> targets;
    for (int i = 0; i < nstate; i++) {
        const int k = map_kind[i], ix = map_index[i];
        const std::string who = "write map, column " + std::to_string(i);
        if (k < -1 || k > 4) { c->err = who + ": kind " + std::to_string(k) + " outside -1..4"; return MONORTM_EARG; }
        long long off = 0;
        if (k == -1) {
            if (ix < -1 || ix > nlay_max) { c->err = who + ": index outside -1.." + std::to_string(nlay_max); return MONORTM_EARG; }
        } else if (k == 4) {
            if (!tmpsfc_a && !tmpsfc_b) { c->err = who + " writes TMPSFC, and both pointers are null"; return MONORTM_EARG; }
        } else {
            if (ix < 0 || ix >= nlay_max + (k == 1)) { c->err = who + ": index " + std::to_string(ix) + " outside " + names[k]; return MONORTM_EARG; }
            if (k == 2 && (map_mol[i] < 0 || map_mol[i] >= nmol)) { c->err = who + ": molecule outside 0.." + std::to_string(nmol - 1); return MONORTM_EARG; }
            off = k == 2 ? (long long)ix * nmol + map_mol[i] : ix;
            if (!arr[k]) { c->err = who + " writes " + names[k] + ", which is null"; return MONORTM_EARG; }
            if (off >= stride[k]) { c->err = who + ": element " + std::to_string(off) + " outside the stride of " + names[k]; return MONORTM_EARG; }
        }
        if (k >= 0) targets.push_back(((long long)k << 40) + off);
        map[i] = k; map[nstate + i] = ix; map[2 * (size_t)nstate + i] = k == 2 ? map_mol[i] : 0;
    }
    std::sort(targets.begin(), targets.end());
    if (std::adjacent_find(targets.begin(), targets.end()) != targets.end()) {
        c->err = "write map: two written columns share a target (give the earlier one kind -1)";
        return MONORTM_EARG;
    }
    if (int rcd = check_device(c)) return rcd;
    hipStream_t s = (hipStream_t)stream;
    if (map != c->oe_wmap_host) {   // as the state map of monortm_hip_oe_step_dev travels
        HIPCHK(c, hipStreamSynchronize(s));
        c->oe_wmap_host.clear();
        HIPCHK(c, grow(&c->oe_wmap, &c->oe_wmap_ints, map.size(), sizeof(int)));
        HIPCHK(c, hipMemcpy(c->oe_wmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
        c->oe_wmap_host = map;
    }
    OeScatterArgs a{};
    a.nprof = nprof; a.nstate = nstate; a.nmol = nmol; a.box_per_profile = box_per_profile;
    a.wmap = static_cast<const int *>(c->oe_wmap); a.nlay = nlay; a.done = done;
    a.x_src = (const double *)x_src; a.x_fallback = (const double *)x_fallback; a.lo = (const double *)lo; a.hi = (const double *)hi;
    a.T = (double *)T; a.TZ = (double *)TZ; a.WKL = (double *)WKL; a.CLW = (double *)CLW; a.tmpsfc_a = (double *)tmpsfc_a; a.tmpsfc_b = (double *)tmpsfc_b;
    a.t_stride = (size_t)t_stride; a.tz_stride = (size_t)tz_stride; a.wkl_stride = (size_t)wkl_stride; a.clw_stride = (size_t)clw_stride;
    a.trial_ok = trial_ok;
    HIPCHK(c, launch_oe_scatter(a, s));
    return MONORTM_OK;
}

int monortm_hip_oe_accept_dev(void *ctx, int nprof, int nmeas, int nstate, const void *Y_trial, const void *y_obs, const void *Se,
                              int se_kind, int se_per_profile, const void *x_trial, const void *c_trial, const void *xa,
                              const int *step_status, const int *trial_ok, double up, double down, double gamma_first, double gamma_floor,
                              double gamma_max, double conv, int last, void *x_cur, void *c_cur, void *J_cur, void *gamma, int *done,
                              int *n_acc, int *n_rej, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return null_ctx();
    if (!c->shards.empty()) return multi_only_host(c);
    if (c->real_kind != 8) { c->err = "monortm_hip_oe_accept_dev needs a real_kind = 8 context"; return MONORTM_EUNSUPPORTED; }
    if (nprof < 1) { c->err = "bad nprof"; return MONORTM_EARG; }
    if (nmeas < 1 || nmeas > kOeMaxMeas) { c->err = "nmeas outside 1.." + std::to_string(kOeMaxMeas); return MONORTM_EARG; }
    if (nstate < 1 || nstate > kOeMaxState) { c->err = "nstate outside 1.." + std::to_string(kOeMaxState); return MONORTM_EARG; }
    if (int rc = oe_check_kind(c, se_kind)) return rc;
    if (se_per_profile != 0 && se_per_profile != 1) { c->err = "se_per_profile must be 0 or 1"; return MONORTM_EARG; }
    if (any_null({Y_trial, y_obs, Se, x_trial, c_trial, xa, step_status, trial_ok, x_cur, c_cur, J_cur, gamma, done, n_acc, n_rej})) {
        c->err = "null array argument";
        return MONORTM_EARG;
    }
    // (written so that a NaN fails every test)
    if (!(up >= 1.) || !(down >= 0. && down <= 1.) || !(gamma_first > 0.) || !(gamma_floor >= 0.) || !(gamma_max >= 0.) || !(conv >= 0.) ||
        !std::isfinite(up) || !std::isfinite(gamma_first)) {
        c->err = "needs up >= 1, 0 <= down <= 1, gamma_first > 0, gamma_floor >= 0, gamma_max >= 0, conv >= 0";
        return MONORTM_EARG;
    }
    if (int rcd = check_device(c)) return rcd;
    OeAcceptArgs a{};
    a.nprof = nprof; a.nmeas = nmeas; a.nstate = nstate; a.se_kind = se_kind; a.se_per_profile = se_per_profile; a.last = last != 0;
    a.Y_trial = (const double *)Y_trial; a.y_obs = (const double *)y_obs; a.se = (const double *)Se; a.x_trial = (const double *)x_trial;
    a.c_trial = (const double *)c_trial; a.xa = (const double *)xa; a.step_status = step_status; a.trial_ok = trial_ok;
    a.up = up; a.down = down; a.gamma_first = gamma_first; a.gamma_floor = gamma_floor; a.gamma_max = gamma_max; a.conv = conv;
    a.x_cur = (double *)x_cur; a.c_cur = (double *)c_cur; a.J_cur = (double *)J_cur; a.gamma = (double *)gamma;
    a.done = done; a.n_acc = n_acc; a.n_rej = n_rej;
    HIPCHK(c, launch_oe_accept(a, (hipStream_t)stream));
    return MONORTM_OK;
}

}  // extern "C"
