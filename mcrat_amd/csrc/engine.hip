// engine.hip -- host side of libmcrat_hip.so: the C ABI of include/mcrat_hip.h on top of the kernels.
//
// Owns the HBM residency of one rank's photon list (SoA columns) and of the current hydro frame
// (packed cell records + the exact cell-lookup grid), and drives the per-iteration kernel pair.
// There is no CPU compute path in this file: if HIP is unavailable every entry point fails.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mcrat_hip.h"
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "sightline_plan.hpp"
#include "escape_plan.hpp"
#include "resample_plan.hpp"
#include "events_plan.hpp"
#include "fit_plan.hpp"
#include "radfield_plan.hpp"
#include "comoving_plan.hpp"
#include "analysis_plan.hpp"
#include "photon_cols.hpp"
#include "photon_plan.hpp"
#include "rng.hpp"

using namespace mcrat;

static_assert(sizeof(mcrat_hip_photon) == 176, "struct photon layout (Src/mcrat.h:142-171) must be 176 bytes");
static_assert(offsetof(mcrat_hip_photon, num_scatt) == 128 && offsetof(mcrat_hip_photon, recalc_properties) == 136 &&
              offsetof(mcrat_hip_photon, weight) == 144 && offsetof(mcrat_hip_photon, nearest_block_index) == 152 &&
              offsetof(mcrat_hip_photon, time_to_scatter) == 160 && offsetof(mcrat_hip_photon, total_optical_depth) == 168,
              "struct photon field offsets");
static_assert(sizeof(LoopState) == 256, "LoopState is one 256-B record");
// the column table of photon_plan.hpp is in the order the loop kernels number the columns (photon_cols.hpp)
static_assert(N_PHOTON_COLS == N_DOUBLE_COLS && N_BLOCK_COLS == N_DOUBLE_COLS + 1, "the block: PhotonDev's double columns and ListCols::draw_log");
#define MCRAT_X(name, K) static_assert(PHOTON_COLS[K] == &PhotonDev::name, "PHOTON_COLS[" #K "] is not PhotonDev::" #name);
MCRAT_DOUBLE_COLS(MCRAT_X)
#undef MCRAT_X
static_assert(sizeof(OutputCols::col) / sizeof(double *) == N_OUTPUT_COLS, "OUTPUT_COLS names the caller's member for every column of OutputCols");

struct mcrat_hip_ctx {
    mcrat_hip_config cfg;
    KernelConfig kc;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;

    // photons
    PhotonDev ph{};
    PhotonLayout ph_lay{};            // the block at ph_buf (photon_plan.hpp); ph is it bound, a view's ph a window of its pool's
    void *ph_buf = nullptr;
    size_t ph_bytes = 0;
    void *ph_snap = nullptr;          // mcrat_hip_snapshot_photons
    void *ph_cap = nullptr;           // mcrat_hip_pool_run_frames with capture_frames: the lists as frames 0 .. n_frames - 2 left them, ph_bytes each
    size_t ph_cap_bytes = 0;
    int cap_frames = 0;               // how many of them the last plan filled
    int selected_frame = -1;          // mcrat_hip_pool_select_frame: the read entry points look at that capture (c->ph shifted), -1: the live lists
    PhotonDev ph_live{};
    size_t ph_snap_bytes = 0;
    bool have_photons = false;
    void *aos_buf = nullptr;          // device copy of the caller's struct photon records (mcrat_hip_set_photons / get_photons)
    void *pin_ring[2] = {nullptr, nullptr};   // pinned staging for uploads gathered from many host buffers (mcrat_hip_pool_set_photons)
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    size_t aos_bytes = 0;
    int step_blocks = 0;
    Cand *partials = nullptr;
    size_t partials_bytes = 0;
    Shortlist *shortlist = nullptr;

    // hydro
    HydroDev hy{};
    void *hy_buf = nullptr;
    size_t hy_bytes = 0;
    bool have_hydro = false;
    void *grid_buf = nullptr;          // bucket records, bucket lists (+ build scratch)
    size_t grid_bytes = 0;
    unsigned *grid_count = nullptr;    // per-bucket counters of the device build
    size_t grid_count_cap = 0;
    unsigned long long *d_grid_total = nullptr;
    void *d_cs_hook = nullptr;                 // CsFrame of the cyclo-synchrotron frame driver
    void *d_cs_args = nullptr;                 // CsHookArgs of the pool's frame driver
    HydroCols hcol{};                  // the frame as struct hydro_dataframe's columns (set_hydro / ingest), kept for get_hydro
    void *hcol_buf = nullptr;
    size_t hcol_bytes = 0;
    int hcol_M = 0;
    void *raw_buf = nullptr;           // device copy of a reader's buffers (mcrat_hip_ingest_*)
    size_t raw_bytes = 0;

    // TAU_CALCULATION == TABLE
    double *d_hot_table = nullptr;
    int hot_n_ph_e = 0, hot_n_t = 0;
    int hot_fallback_calls = 500000;   // hot_x_section.c:348
    double hot_grid[4] = {0, 0, 0, 0};          // log10 photon energy min/max, log10 theta min/max
    int *d_table_fallbacks = nullptr;
    int hot_creating = 0;              // a thread is inside mcrat_hip_create_hot_cross_section on this context (read and written atomically)

    // loop
    LoopState *d_state = nullptr;
    LoopState *h_state = nullptr;     // pinned
    bool frame_open = false;
    int find_switch = 1;
    RngKey key{0, 0, 0};
    long long frame_photon_steps = 0;
    mcrat_hip_ctx *hydro_owner = nullptr;   // mcrat_hip_share_hydro: the staged frame (and cross-section table) are another context's
    std::vector<mcrat_hip_ctx *> hydro_sharers;   // ... and, on that context, who reads its frame: they are cut loose before it changes or goes
    void *d_fast = nullptr;           // FAST mode's counters (FastCounts)
    bool pending_applied = false;     // step_locate_sample has applied the pending advance that LoopState still lists
    bool rank_current = false;        // a view whose frame rank_loop_kernel has run: it leaves no pending advance (until the next begin_frame)

    // virtual ranks (cfg.virtual_rank_photons > 0): one LoopState per list
    int n_ranks = 0;
    int rank_block = 256;             // threads per list of the next launches (choose_rank_block)
    bool rank_fuse = true;            // ... and whether they use the build with the fused pass
    // the random stream as an input (mcrat_hip_set_rng_tape): device copy of the caller's uniforms, the position reached, an error word
    double *d_tape = nullptr;
    long long tape_n = 0;
    long long *d_tape_cursor = nullptr;   // {cursor, error word} in one 16-byte block
    // ... for the lists of a rank pool (mcrat_hip_pool_set_rng_tapes): every list's tape concatenated, one TapeList per list; a pool with
    // d_pool_tapes runs every frame through the tape build (launch_rank_loop_tape)
    double *d_pool_tape = nullptr;
    TapeList *d_pool_tapes = nullptr;
    int fast_auto_windows = 32;       // FAST mode with fast_windows <= 0: the refresh cadence, from what the last FAST frame looked like (fast_cadence)
    bool rank_block_fixed = false;
    double rank_passes_per_list = 0;  // of the last completed frame
    LoopState *d_rstates = nullptr;
    LoopState *h_rstates = nullptr;   // pinned
    size_t d_rstates_bytes = 0, h_rstates_bytes = 0;

    // rank pool (mcrat_hip_pool_*): the photon arrays hold n_ranks lists of up to rank_stride slots, each with its own length,
    // seed, stream and clock -- the reference's MPI ranks, adopted by one GPU.  List r is reached through a *view*: a context
    // whose columns, LoopState and scratch are windows into this one, so that every per-list entry point (injection, reductions,
    // output columns, checkpoint records, ...) works on one rank's list unchanged.
    bool is_pool = false;
    int rank_stride = 0;              // slots reserved per list (pool), or cfg.virtual_rank_photons
    std::vector<mcrat_hip_ctx *> views;
    std::vector<int> snap_lens;       // the lists' lengths when mcrat_hip_snapshot_photons was taken
    RankDesc *d_desc = nullptr;
    RankDesc *h_desc = nullptr;       // pinned
    void *d_fq = nullptr, *h_fq = nullptr;   // the frame queue's block (mcrat_hip_pool_run_frames): order, items, hydro frames, list descriptions, ticket, frames_done, records; pinned mirror
    size_t fq_bytes = 0;
    std::vector<int> fq_first, fq_last, fq_hy_of_frame, fq_stalled;   // ... and that call's scratch, kept from call to call
    std::vector<HydroDev> fq_hyv;
    std::vector<const mcrat_hip_ctx *> fq_hy_ctx;
    RankDeviceInfo dev{0, 0};         // the context's device and its CU count, read once (mcrat_hip_init); cus == 0: not known, the launchers ask
    mcrat_hip_ctx *parent = nullptr;  // this context is the view of list view_rank of `parent`
    int view_rank = -1;
    uint32_t view_stream = 0;

    // one list over several GPUs, one clock (mcrat_hip_shared_clock_*)
    int sc_world = 0, sc_rank = 0;
    ScState *d_sc = nullptr;
    ScProposal *sc_send = nullptr, *sc_recv = nullptr;
    // device-initiated exchange (mcrat_hip_shared_clock_attach_device): fine-grained receive buffer (2 x world proposals) and stamps
    bool sc_device = false, sc_peers_set = false;
    bool sc_fold = true;              // device exchange: push and wait run inside the propose and resolve kernels (MCRAT_HIP_SC_FOLD=0: as launches of their own)
    unsigned long long *sc_flags = nullptr;
    ScProposal *sc_gather = nullptr;   // the round's proposals of all ranks, copied out of the receive buffer's current half: what resolve reads
    ScPeers sc_peers{};
    bool sc_own_send = false, sc_own_recv = false;

    // scratch
    ReducePartial *d_red = nullptr;
    ReducePartial *h_red = nullptr;   // pinned
    static constexpr int RED_BLOCKS = 512;
    // the device blocks of the analysis products, each laid out by its plan header: mcrat_hip_observe (the cube, the per-observer counters and the
    // staged inputs), mcrat_hip_sightline_* (the output block and the caller's rays), mcrat_hip_radiation_field (head, accumulator and staged
    // edges), mcrat_hip_observe_sky (as observe), mcrat_hip_comoving_field (as radiation_field), mcrat_hip_observe_escaping (planes, counters, head, staged
    // inputs and the compacted list), mcrat_hip_observe_sky_resampled (as observe, with a third counter), mcrat_hip_observe_events (head, staged
    // observers, count table, row columns, the sort's buffers), mcrat_hip_fit_spectra (the edges, log_e, the spectra and the output columns).  Nine
    // products.  A view uses its pool's (analysis_block).
    enum AnalysisBlock { BLOCK_OBSERVE = 0, BLOCK_SIGHTLINE, BLOCK_RADFIELD, BLOCK_SKY, BLOCK_COMOVING, BLOCK_ESCAPE, BLOCK_RESAMPLE, BLOCK_EVENTS, BLOCK_FIT, N_ANALYSIS_BLOCKS };
    struct DeviceBlock { void *buf = nullptr; size_t bytes = 0; } analysis[N_ANALYSIS_BLOCKS];
    int obs_path = 0;                 // the accumulation path of the last observation (ObservePath)
    int rf_path = 0;                  // the accumulation path of the last radiation field (ObservePath)
    int sky_path = 0;                 // the accumulation path of the last sky observation (ObservePath)
    int cf_path = 0;                  // the accumulation path of the last comoving field (ObservePath)
    int esc_path = 0;                 // the accumulation path of the last escape-weighted observation (ObservePath)
    int rs_path = 0;                  // the accumulation path of the last resampled sky observation (ResamplePath)

    // profiling
    std::vector<hipEvent_t> ev;
    double prof_step_ms = 0, prof_event_ms = 0;
    long long prof_launches = 0;

    // graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_batch = 0;
};

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return (e_ == hipErrorOutOfMemory) ? MCRAT_HIP_ENOMEM : MCRAT_HIP_EHIP;                \
        }                                                                                          \
    } while (0)

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static bool env_flag(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }      // an environment switch: set, and not to 0
// a device buffer that only grows: room for `need` bytes at *buf -- the buffer as it is when it has them, a new one of `need` bytes when not (the
// contents go; the caller has made sure that nothing on the device still reads them)
static int ensure_device_bytes(mcrat_hip_ctx *c, void **buf, size_t *bytes, size_t need)
{
    if (*buf && *bytes < need) { HIPCHK(c, hipFree(*buf)); *buf = nullptr; *bytes = 0; }
    if (!*buf) { HIPCHK(c, hipMalloc(buf, need)); *bytes = need; }
    return MCRAT_HIP_OK;
}
// ... and its pinned-host twin
static int ensure_host_bytes(mcrat_hip_ctx *c, void **buf, size_t *bytes, size_t need)
{
    if (*buf && *bytes < need) { HIPCHK(c, hipHostFree(*buf)); *buf = nullptr; *bytes = 0; }
    if (!*buf && need) { HIPCHK(c, hipHostMalloc(buf, need, hipHostMallocDefault)); *bytes = need; }
    return MCRAT_HIP_OK;
}

// a temporary device array of one call: freed where its scope ends, whichever way the call leaves it
template <class T>
struct DeviceTemp {
    T *p = nullptr;
    size_t cap = 0;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp &) = delete;
    ~DeviceTemp() { (void)hipFree(p); }
    hipError_t alloc(size_t count) { cap = count; return hipMalloc((void **)&p, sizeof(T) * count); }       // once
    // room for `count`: a larger array when there is not (the contents go)
    hipError_t reserve(size_t count) { if (count <= cap) return hipSuccess; (void)hipFree(p); p = nullptr; return alloc(count); }
    operator T *() const { return p; }
};

static InjectParams inject_params(const mcrat_hip_ctx *c, const Region &slab)
{
    return InjectParams{c->kc.dimensions, c->kc.geometry, slab.rmin, slab.rmax, slab.tmin, slab.tmax, inject_num_dens_coeff(slab.wien != 0), slab.wien};
}
// what the emission kernels and the hook are given; the shell is left empty (the hook has none: emit_into)
static CsEmitParams cs_emit_params(const mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs)
{
    return CsEmitParams{c->kc.dimensions, c->kc.geometry, cs->b_field_calc, cs->epsilon_b, 0.0, 0.0, 0.0, 0.0};
}
static void emit_into(CsEmitParams &p, const Region &shell) { p.rmin = shell.rmin; p.rmax = shell.rmax; p.theta_min = shell.tmin; p.theta_max = shell.tmax; }
// One region (p: a slab's InjectParams or a shell's CsEmitParams) for the lists of a pool that share it: its cells flagged in c->grid_count and counted,
// *n_cells of them, room for their records in d_cells, and write() -- the region's launch_region_write -- scans the flags and writes the records
template <class Params, class Cell, class Write>
static int pool_region_cells(mcrat_hip_ctx *c, const Params &p, DeviceTemp<Cell> &d_cells, int *n_cells, Write write)
{
    if (launch_region_flag(p, c->hy, c->grid_count, c->d_grid_total, n_cells, c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
    if (d_cells.reserve((size_t)*n_cells) != hipSuccess) return MCRAT_HIP_ENOMEM;
    return write() == hipSuccess ? MCRAT_HIP_OK : MCRAT_HIP_EHIP;
}

static void drop_graph(mcrat_hip_ctx *c)
{
    if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
    if (c->graph) { (void)hipGraphDestroy(c->graph); c->graph = nullptr; }
    c->graph_batch = 0;
}

static void sync_views(mcrat_hip_ctx *c);
static int view_refuses(mcrat_hip_ctx *c, const char *what);
static int capture_refuses(mcrat_hip_ctx *c, const char *what);
static void release_shared_hydro(mcrat_hip_ctx *c);
static int ensure_counts(mcrat_hip_ctx *c, size_t n);

extern "C" const char *mcrat_hip_version(void) { return "mcrat_hip 0.1 (gfx950, abi 1)"; }

extern "C" const char *mcrat_hip_strerror(int code)
{
    switch (code) {
    case MCRAT_HIP_OK: return "ok";
    case MCRAT_HIP_EINVAL: return "invalid argument or unsupported switch combination";
    case MCRAT_HIP_ENODEV: return "no usable HIP device";
    case MCRAT_HIP_ENOMEM: return "out of memory";
    case MCRAT_HIP_EHIP: return "HIP runtime error";
    case MCRAT_HIP_ESTATE: return "call out of order";
    case MCRAT_HIP_EREFUSED: return "refused as the reference refuses it (nothing was changed)";
    default: return "unknown error";
    }
}

extern "C" const char *mcrat_hip_last_error(const mcrat_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

static bool geometry_supported(int dims, int geom)
{
    if (dims == DIM_TWO || dims == DIM_TWO_POINT_FIVE)
        return geom == GEOM_CARTESIAN || geom == GEOM_CYLINDRICAL || geom == GEOM_SPHERICAL;
    if (dims == DIM_THREE) return geom == GEOM_CARTESIAN || geom == GEOM_SPHERICAL || geom == GEOM_POLAR;
    return false;
}

extern "C" int mcrat_hip_init(mcrat_hip_ctx **out, const mcrat_hip_config *cfg)
{
    if (!out || !cfg) return MCRAT_HIP_EINVAL;
    *out = nullptr;
    if (cfg->abi_version != MCRAT_HIP_ABI_VERSION) return MCRAT_HIP_EINVAL;
    if (!geometry_supported(cfg->dimensions, cfg->geometry)) return MCRAT_HIP_EINVAL;
    if (cfg->tau_calculation != MCRAT_HIP_TAU_DIRECT && cfg->tau_calculation != MCRAT_HIP_TAU_TABLE) return MCRAT_HIP_EINVAL;
    if (cfg->virtual_rank_photons < 0) return MCRAT_HIP_EINVAL;
    // with the switch on the list changes length inside the loop; one list per context, driven by
    // mcrat_hip_scatter_frame_cyclosynch
    if (cfg->cyclosynchrotron_switch != 0 && (cfg->cyclosynchrotron_switch != 1 || cfg->virtual_rank_photons != 0)) return MCRAT_HIP_EINVAL;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return MCRAT_HIP_ENODEV;
    if (hipSetDevice(cfg->device) != hipSuccess) return MCRAT_HIP_ENODEV;

    mcrat_hip_ctx *c = new (std::nothrow) mcrat_hip_ctx();
    if (!c) return MCRAT_HIP_ENOMEM;
    c->cfg = *cfg;
    c->dev.device = cfg->device;
    if (hipDeviceGetAttribute(&c->dev.cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || c->dev.cus < 0) { (void)hipGetLastError(); c->dev.cus = 0; }
    if (c->cfg.iterations_per_sync <= 0) c->cfg.iterations_per_sync = 256;
    c->kc.dimensions = cfg->dimensions;
    c->kc.geometry = cfg->geometry;
    c->kc.stokes = cfg->stokes_switch ? 1 : 0;
    c->kc.table = cfg->tau_calculation == MCRAT_HIP_TAU_TABLE ? 1 : 0;
    c->key.stream = cfg->rng_stream & 0xffffffu;

    auto fail = [&](int code) { mcrat_hip_destroy(c); return code; };
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(MCRAT_HIP_ENODEV);
        c->own_stream = true;
    }
    if (hipMalloc((void **)&c->d_state, sizeof(LoopState)) != hipSuccess) return fail(MCRAT_HIP_ENOMEM);
    if (hipMalloc((void **)&c->d_table_fallbacks, sizeof(int)) != hipSuccess) return fail(MCRAT_HIP_ENOMEM);
    if (hipMemset(c->d_table_fallbacks, 0, sizeof(int)) != hipSuccess) return fail(MCRAT_HIP_ENODEV);
    if (hipHostMalloc((void **)&c->h_state, sizeof(LoopState), hipHostMallocDefault) != hipSuccess) return fail(MCRAT_HIP_ENOMEM);
    if (hipMalloc((void **)&c->d_red, sizeof(ReducePartial) * mcrat_hip_ctx::RED_BLOCKS) != hipSuccess) return fail(MCRAT_HIP_ENOMEM);
    if (hipHostMalloc((void **)&c->h_red, sizeof(ReducePartial) * mcrat_hip_ctx::RED_BLOCKS, hipHostMallocDefault) != hipSuccess)
        return fail(MCRAT_HIP_ENOMEM);
    memset(c->h_state, 0, sizeof(LoopState));
    c->h_state->done = 1;
    c->h_state->skip_idx = -1;
    if (hipMemcpy(c->d_state, c->h_state, sizeof(LoopState), hipMemcpyHostToDevice) != hipSuccess) return fail(MCRAT_HIP_ENODEV);
    *out = c;
    return MCRAT_HIP_OK;
}

static void destroy_view(mcrat_hip_ctx *v)
{
    // a view owns nothing but its cyclo-synchrotron hook state, a snapshot and its events; the rest are windows into the pool
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    if (v->d_cs_hook) (void)hipFree(v->d_cs_hook);
    if (v->d_fast) (void)hipFree(v->d_fast);
    if (v->ph_snap) (void)hipFree(v->ph_snap);
    for (hipEvent_t e : v->ev) (void)hipEventDestroy(e);
    if (v->parent && v->view_rank >= 0 && v->view_rank < (int)v->parent->views.size() && v->parent->views[v->view_rank] == v)
        v->parent->views[v->view_rank] = nullptr;
    delete v;
}

// Contexts that read another one's staged frame (mcrat_hip_share_hydro) hold raw device pointers into its buffers.  Before the owner
// re-stages (the buffers are rewritten in place, or freed when the new frame is larger), replaces its cross-section table or is destroyed,
// every sharer is cut loose: its stream is drained -- a launch of its own may still be reading the frame -- and it is left WITHOUT a frame
// (have_hydro = false: begin_frame / run / share answer MCRAT_HIP_ESTATE until it shares or stages again).  One mutex guards the
// bookkeeping, so that pools driven by their own host threads may share and re-stage; a sharer must not be inside a call of its own
// while its owner re-stages (stage once per hydro frame behind a barrier and share again after it: INTEGRATION.md).
static std::mutex g_share_mutex;
static void sync_views(mcrat_hip_ctx *c);

static void forget_shared_frame(mcrat_hip_ctx *s)          // (g_share_mutex held)
{
    s->hydro_owner = nullptr;
    s->hy = HydroDev{};
    s->hcol = HydroCols{};
    s->hcol_buf = nullptr; s->hcol_M = 0; s->hcol_bytes = 0;
    s->d_hot_table = nullptr;
    s->have_hydro = false;
    s->frame_open = false;
    sync_views(s);
}

static void detach_sharers(mcrat_hip_ctx *owner, const char *why)
{
    std::lock_guard<std::mutex> lock(g_share_mutex);
    for (mcrat_hip_ctx *s : owner->hydro_sharers) {
        if (!s || s->hydro_owner != owner) continue;
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        forget_shared_frame(s);
        s->last_error = std::string("the hydro frame this context shared is gone (its owner ") + why + "): share or stage a frame again";
    }
    owner->hydro_sharers.clear();
}

extern "C" void mcrat_hip_destroy(mcrat_hip_ctx *c)
{
    if (!c) return;
    if (c->parent) { destroy_view(c); return; }
    detach_sharers(c, "was destroyed");
    for (mcrat_hip_ctx *v : c->views)
        if (v) { v->parent = nullptr; destroy_view(v); }
    c->views.clear();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_graph(c);
    if (c->hydro_owner) {                                    // another context's frame: nothing of it is ours to free
        std::lock_guard<std::mutex> lock(g_share_mutex);
        auto &v = c->hydro_owner->hydro_sharers;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
        c->hcol_buf = nullptr; c->d_hot_table = nullptr; c->hydro_owner = nullptr;
    }
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->d_desc) (void)hipFree(c->d_desc);
    if (c->h_desc) (void)hipHostFree(c->h_desc);
    if (c->d_fq) (void)hipFree(c->d_fq);
    if (c->h_fq) (void)hipHostFree(c->h_fq);
    if (c->ph_buf) (void)hipFree(c->ph_buf);
    for (int k = 0; k < 2; ++k) { if (c->pin_ring[k]) (void)hipHostFree(c->pin_ring[k]); if (c->pin_ev[k]) (void)hipEventDestroy(c->pin_ev[k]); }
    if (c->ph_snap) (void)hipFree(c->ph_snap);
    if (c->ph_cap) (void)hipFree(c->ph_cap);
    if (c->aos_buf) (void)hipFree(c->aos_buf);
    if (c->hy_buf) (void)hipFree(c->hy_buf);
    if (c->grid_buf) (void)hipFree(c->grid_buf);
    if (c->hcol_buf) (void)hipFree(c->hcol_buf);
    if (c->raw_buf) (void)hipFree(c->raw_buf);
    if (c->grid_count) (void)hipFree(c->grid_count);
    if (c->d_grid_total) (void)hipFree(c->d_grid_total);
    if (c->d_cs_hook) (void)hipFree(c->d_cs_hook);
    if (c->d_cs_args) (void)hipFree(c->d_cs_args);
    if (c->d_fast) (void)hipFree(c->d_fast);
    if (c->partials) (void)hipFree(c->partials);
    if (c->shortlist) (void)hipFree(c->shortlist);
    if (c->d_hot_table) (void)hipFree(c->d_hot_table);
    if (c->d_tape) (void)hipFree(c->d_tape);
    if (c->d_tape_cursor) (void)hipFree(c->d_tape_cursor);
    if (c->d_pool_tape) (void)hipFree(c->d_pool_tape);
    if (c->d_pool_tapes) (void)hipFree(c->d_pool_tapes);
    if (c->d_table_fallbacks) (void)hipFree(c->d_table_fallbacks);
    if (c->d_sc) (void)hipFree(c->d_sc);
    if (c->sc_own_send && c->sc_send) (void)hipFree(c->sc_send);
    if (c->sc_own_recv && c->sc_recv) (void)hipFree(c->sc_recv);
    if (c->sc_flags) (void)hipFree(c->sc_flags);
    if (c->sc_gather) (void)hipFree(c->sc_gather);
    if (c->d_rstates) (void)hipFree(c->d_rstates);
    if (c->h_rstates) (void)hipHostFree(c->h_rstates);
    if (c->d_state) (void)hipFree(c->d_state);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->d_red) (void)hipFree(c->d_red);
    if (c->h_red) (void)hipHostFree(c->h_red);
    for (const auto &b : c->analysis)
        if (b.buf) (void)hipFree(b.buf);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// HIP's current device is a property of the host thread: a thread other than the one that created the context must select the context's
// device before it calls into the library (allocations made on the way would otherwise land on the thread's default device)
extern "C" int mcrat_hip_bind_thread(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (hipSetDevice(c->cfg.device) != hipSuccess) return MCRAT_HIP_ENODEV;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_synchronize(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" size_t mcrat_hip_device_bytes(const mcrat_hip_ctx *c)
{
    if (!c) return 0;
    size_t analysis = 0;
    for (const auto &b : c->analysis) analysis += b.bytes;
    return c->ph_bytes + c->hy_bytes + c->grid_bytes + c->grid_count_cap * sizeof(unsigned) + sizeof(Shortlist) + sizeof(LoopState) + c->partials_bytes +
           sizeof(ReducePartial) * mcrat_hip_ctx::RED_BLOCKS + analysis;
}

extern "C" int mcrat_hip_create_hot_cross_section(mcrat_hip_ctx *c, double *thermal_table, int n_ph_e, int n_t, double log_ph_e_min,
                                                  double log_ph_e_max, double log_t_min, double log_t_max, long long calls, uint64_t seed)
{
    if (!c || !thermal_table || n_ph_e < 1 || n_t < 1 || n_ph_e > 100000 || n_t > 100000 || calls < 1 || !(log_ph_e_max > log_ph_e_min) ||
        !(log_t_max > log_t_min))
        return MCRAT_HIP_EINVAL;
    const size_t count = (size_t)(n_ph_e + 1) * (size_t)(n_t + 1);
    if (count > 0x7fffffffull) return MCRAT_HIP_EINVAL;
    double *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, count * sizeof(double)));
    HotTableParams p{n_ph_e, n_t, log_ph_e_min, log_ph_e_max, log_t_min, log_t_max, calls, (unsigned long long)seed};
    __atomic_store_n(&c->hot_creating, 1, __ATOMIC_RELEASE);      // mcrat_hip_eval_function refuses THERMAL_CROSS_SECTION meanwhile
    hipError_t e = launch_hot_table(p, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(thermal_table, d, count * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    __atomic_store_n(&c->hot_creating, 0, __ATOMIC_RELEASE);
    (void)hipFree(d);
    HIPCHK(c, e);
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- hydro staging
// (the host's rules -- the bucket grid's plan and its host build, the buffers' layouts, an ingest's slab and box table -- are hydro_plan.hpp)

static void apply_hot_table(mcrat_hip_ctx *c)
{
    HydroDev &hy = c->hy;
    const bool table = c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && c->d_hot_table;
    hy.hot_table = table ? c->d_hot_table : nullptr;
    hy.hot_n_ph_e = c->hot_n_ph_e; hy.hot_n_t = c->hot_n_t;
    hy.hot_e0 = c->hot_grid[0]; hy.hot_t0 = c->hot_grid[2];
    // the grid steps as hot_x_section.c:464 forms them
    hy.hot_de = table ? (c->hot_grid[1] - c->hot_grid[0]) / c->hot_n_ph_e : 0.0;
    hy.hot_dt = table ? (c->hot_grid[3] - c->hot_grid[2]) / c->hot_n_t : 0.0;
    hy.table_fallbacks = c->d_table_fallbacks;
    hy.hot_fallback_calls = c->hot_fallback_calls;
}

extern "C" int mcrat_hip_table_fallback_calls(mcrat_hip_ctx *c, int calls)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (calls > 0) {
        c->hot_fallback_calls = calls;
        apply_hot_table(c);
        drop_graph(c);
        sync_views(c);
    }
    return c->hot_fallback_calls;
}

extern "C" int mcrat_hip_set_hot_cross_section(mcrat_hip_ctx *c, const double *thermal_table, int n_ph_e, int n_t,
                                               double log_ph_e_min, double log_ph_e_max, double log_t_min, double log_t_max)
{
    if (!c || !thermal_table || n_ph_e < 1 || n_t < 1 || !(log_ph_e_max > log_ph_e_min) || !(log_t_max > log_t_min)) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "set_hot_cross_section");
    if (c->cfg.tau_calculation != MCRAT_HIP_TAU_TABLE) { c->last_error = "the context was created with TAU_CALCULATION == DIRECT"; return MCRAT_HIP_ESTATE; }
    const size_t count = (size_t)(n_ph_e + 1) * (size_t)(n_t + 1);
    for (size_t k = 0; k < count; ++k)
        if (!(thermal_table[k] == thermal_table[k])) { c->last_error = "NaN in the cross-section table"; return MCRAT_HIP_EINVAL; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release_shared_hydro(c);
    detach_sharers(c, "replaced its cross-section table");   // they read this table too
    if (c->d_hot_table) { (void)hipFree(c->d_hot_table); c->d_hot_table = nullptr; }
    HIPCHK(c, hipMalloc((void **)&c->d_hot_table, count * sizeof(double)));
    HIPCHK(c, hipMemcpy(c->d_hot_table, thermal_table, count * sizeof(double), hipMemcpyHostToDevice));
    c->hot_n_ph_e = n_ph_e; c->hot_n_t = n_t;
    c->hot_grid[0] = log_ph_e_min; c->hot_grid[1] = log_ph_e_max; c->hot_grid[2] = log_t_min; c->hot_grid[3] = log_t_max;
    apply_hot_table(c);
    drop_graph(c);
    sync_views(c);
    return MCRAT_HIP_OK;
}

static int ensure_aos(mcrat_hip_ctx *c, size_t bytes);
static int flush_pending(mcrat_hip_ctx *c);

// rank pool: the views read the pool's hydro frame (and cross-section table) through copies of its descriptors
static void sync_views(mcrat_hip_ctx *c)
{
    for (mcrat_hip_ctx *v : c->views) {
        if (!v) continue;
        v->hy = c->hy;
        v->hcol = c->hcol; v->hcol_buf = c->hcol_buf; v->hcol_M = c->hcol_M;
        v->have_hydro = c->have_hydro;
        v->d_hot_table = c->d_hot_table; v->hot_n_ph_e = c->hot_n_ph_e; v->hot_n_t = c->hot_n_t;
        v->hot_fallback_calls = c->hot_fallback_calls;
        for (int k = 0; k < 4; ++k) v->hot_grid[k] = c->hot_grid[k];
        drop_graph(v);
    }
}

// per-context scratch: `n` counters and the 8-byte total.  A view borrows its pool's (one stream, one call at a time): a thousand
// views must not hold a thousand cell-sized arrays.
static int ensure_counts(mcrat_hip_ctx *c, size_t n)
{
    if (c->parent) {
        int rc = ensure_counts(c->parent, n);
        c->grid_count = c->parent->grid_count; c->grid_count_cap = c->parent->grid_count_cap; c->d_grid_total = c->parent->d_grid_total;
        return rc;
    }
    if (!c->d_grid_total) HIPCHK(c, hipMalloc((void **)&c->d_grid_total, sizeof(unsigned long long)));
    if (c->grid_count_cap < n) {
        if (c->grid_count) { HIPCHK(c, hipFree(c->grid_count)); c->grid_count = nullptr; c->grid_count_cap = 0; }
        HIPCHK(c, hipMalloc((void **)&c->grid_count, sizeof(unsigned) * n));
        c->grid_count_cap = n;
    }
    return MCRAT_HIP_OK;
}

static int view_refuses(mcrat_hip_ctx *c, const char *what)
{
    c->last_error = std::string(what) + ": a rank view shares its pool's hydro frame; call this on the pool context";
    return MCRAT_HIP_ESTATE;
}

// While a captured frame is selected (mcrat_hip_pool_select_frame) the pool's columns are that capture's: the read entry points are meant to look
// there, every pool entry point that writes photons or loop state refuses -- it would write into the capture
static int capture_refuses(mcrat_hip_ctx *c, const char *what)
{
    if (c->selected_frame < 0) return MCRAT_HIP_OK;
    c->last_error = std::string(what) + ": a captured frame is selected (mcrat_hip_pool_select_frame(pool, -1) first)";
    return MCRAT_HIP_ESTATE;
}

// Staging a frame: its per-cell records and its cell-lookup grid into c->hy_buf and c->grid_buf, then c->hy.  The product path takes the device
// columns c->hcol and works on the device -- stage_cells_kernel (ingest.hip) + grid_build.hip; the host only plans the bucket grid from the mesh
// statistics the kernel reduces.  With the caller's host columns (MCRAT_HIP_HOST_GRID=1) the staging loop and the grid build run on the host: the
// cross-check of the device path (tests/test_gpu_parity.py).  Each is a sequence of steps over one HydroStage (stage_hydro_device, stage_hydro_host);
// they share the buffers' steps and end in the same publish_grid and finish_frame.
namespace {

struct HydroStage {
    mcrat_hip_ctx *c;
    int M, naxes;
    CellLayout cells{};               // c->hy_buf
    GridLayout grid{};                // c->grid_buf
    GridScale scale{};                // device build: the grid up to its scale factor, from the staging kernel's statistics
    GridPlan plan{};                  // the grid that is built, with its buckets and list entries
    long long nb = 0, entries = 0;
    size_t covered_ints = 0;          // the covered-octant table's ints (covered_table_ints); 0: the grid has none
    bool any_hot = false;             // a cell has T >= 1e7 K: the frame gets the k2e column
    template <class T> T *cell_at(size_t o) const { return reinterpret_cast<T *>(static_cast<char *>(c->hy_buf) + o); }
    template <class T> T *grid_at(size_t o) const { return reinterpret_cast<T *>(static_cast<char *>(c->grid_buf) + o); }
};
// what the host build keeps between its steps: the caller's columns, the grid, and the per-cell buffer's image (the bucket lists copy from it)
struct HostFrame {
    const mcrat_hip_hydro *h;
    GridHost grid;
    std::vector<char> image;
};

// host build: the whole grid, before anything of the context changes (a mesh it refuses leaves the buffers alone)
int host_build_grid(HydroStage &s, HostFrame &hf)
{
    const mcrat_hip_hydro *h = hf.h;
    const double *ctr[3] = {h->r0, h->r1, h->r2}, *size[3] = {h->r0_size, h->r1_size, h->r2_size};
    if (!build_grid(ctr, size, s.M, s.naxes, hf.grid)) { s.c->last_error = "cell-lookup grid: degenerate mesh"; return MCRAT_HIP_EINVAL; }
    s.plan = hf.grid.plan; s.nb = hf.grid.nb; s.entries = (long long)hf.grid.cells.size();
    for (int i = 0; i < s.M; ++i) s.any_hot = s.any_hot || (h->temp[i] >= 1e7);
    return MCRAT_HIP_OK;
}

int ensure_cell_buffer(HydroStage &s, bool reserve_k2e)
{
    mcrat_hip_ctx *c = s.c;
    s.cells = cell_layout(c->kc.dimensions, s.M, reserve_k2e);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ensure_device_bytes(c, &c->hy_buf, &c->hy_bytes, s.cells.total);
}

// device build: the cells' records from c->hcol, and from the statistics the kernel reduced on the way the grid up to its scale
int stage_cells_device(HydroStage &s)
{
    mcrat_hip_ctx *c = s.c;
    const CellLayout &l = s.cells;
    const int M = s.M, nblk = stage_cells_blocks(M), stride = plan_stride(M), nsamp = (M + stride - 1) / stride;
    const size_t scratch_bytes = sizeof(StagePartial) * (size_t)nblk + sizeof(double) * 2 * s.naxes * (size_t)nsamp;
    int rc = ensure_aos(c, scratch_bytes);
    if (rc) return rc;
    StagePartial *d_part = static_cast<StagePartial *>(c->aos_buf);
    double *d_samp = reinterpret_cast<double *>(d_part + nblk);
    HIPCHK(c, launch_stage_cells(c->kc.dimensions, c->kc.geometry, c->hcol, M, s.cell_at<CellGeom>(l.geom), l.has_geom2 ? s.cell_at<CellGeom2>(l.geom2) : nullptr,
                                 s.cell_at<CellFluid>(l.fluid), l.has_fluid_c ? s.cell_at<double>(l.fluid_c) : nullptr, s.cell_at<double>(l.temp),
                                 s.cell_at<double>(l.gamma), d_part, d_samp, stride, nsamp, c->stream));
    std::vector<char> hs(scratch_bytes);
    HIPCHK(c, hipMemcpyAsync(hs.data(), c->aos_buf, scratch_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const StagePartial *part = reinterpret_cast<const StagePartial *>(hs.data());
    const MeshStats ms = mesh_stats_from_partials(part, nblk, reinterpret_cast<const double *>(part + nblk), nsamp, s.naxes, &s.any_hot);
    if (!grid_plan_from_stats(ms, M, s.naxes, s.scale)) { c->last_error = "cell-lookup grid: degenerate mesh"; return MCRAT_HIP_EINVAL; }
    return MCRAT_HIP_OK;
}

// host build: the same records from the caller's columns, as the buffer's image, and up
int stage_cells_host(HydroStage &s, HostFrame &hf)
{
    mcrat_hip_ctx *c = s.c;
    const mcrat_hip_hydro *h = hf.h;
    const CellLayout &l = s.cells;
    const int M = s.M;
    hf.image.assign(l.total, 0);
    char *host = hf.image.data();
    CellGeom *geom = reinterpret_cast<CellGeom *>(host + l.geom);
    CellFluid *fluid = reinterpret_cast<CellFluid *>(host + l.fluid);
    double *fc = l.has_fluid_c ? reinterpret_cast<double *>(host + l.fluid_c) : nullptr;
    for (int i = 0; i < M; ++i) {
        geom[i].c0 = h->r0[i]; geom[i].c1 = h->r1[i]; geom[i].s0 = h->r0_size[i]; geom[i].s1 = h->r1_size[i];
        double v[3];
        cell_velocity_staged(c->kc.dimensions, c->kc.geometry, h->v0[i], h->v1[i], l.has_fluid_c ? h->v2[i] : 0.0, h->r1[i], l.has_geom2 ? h->r2[i] : 0.0, v);
        if (fc) fc[i] = v[2];
        cell_staged_operands(v[0], v[1], v[2], h->gamma[i], h->dens_lab[i], fluid[i]);
    }
    if (l.has_geom2) {
        CellGeom2 *g2 = reinterpret_cast<CellGeom2 *>(host + l.geom2);
        for (int i = 0; i < M; ++i) { g2[i].c2 = h->r2[i]; g2[i].s2 = h->r2_size[i]; }
    }
    memcpy(host + l.temp, h->temp, sizeof(double) * M);
    memcpy(host + l.gamma, h->gamma, sizeof(double) * M);
    HIPCHK(c, hipMemcpy(c->hy_buf, host, l.total, hipMemcpyHostToDevice));
    return MCRAT_HIP_OK;
}

void publish_cells(HydroStage &s, const double *dom0, const double *dom1, const double *dom2)
{
    const CellLayout &l = s.cells;
    HydroDev &hy = s.c->hy;
    hy.geom = s.cell_at<const CellGeom>(l.geom);
    hy.geom2 = l.has_geom2 ? s.cell_at<const CellGeom2>(l.geom2) : nullptr;
    hy.fluid = s.cell_at<const CellFluid>(l.fluid);
    hy.temp = s.cell_at<const double>(l.temp);
    hy.fluid_c = l.has_fluid_c ? s.cell_at<const double>(l.fluid_c) : nullptr;
    hy.k2e = s.any_hot ? s.cell_at<const double>(l.k2e) : nullptr;
    hy.gamma = s.cell_at<const double>(l.gamma);
    hy.M = s.M;
    hy.dom0[0] = dom0[0]; hy.dom0[1] = dom0[1];
    hy.dom1[0] = dom1[0]; hy.dom1[1] = dom1[1];
    hy.dom2[0] = dom2[0]; hy.dom2[1] = dom2[1];
}

// device build: the entries a plan's bucket lists would hold (grid_build.hip counts them, per bucket too: c->grid_count)
int count_grid_entries(HydroStage &s, const GridPlan &plan, long long nb, unsigned long long *total)
{
    mcrat_hip_ctx *c = s.c;
    { int rc = ensure_counts(c, (size_t)nb); if (rc) return rc; }
    HIPCHK(c, grid_count(plan, c->hy.geom, c->hy.geom2, s.M, c->grid_count, nb, c->d_grid_total, c->stream));
    HIPCHK(c, hipMemcpyAsync(total, c->d_grid_total, sizeof *total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}
int choose_scale_device(HydroStage &s)
{
    mcrat_hip_ctx *c = s.c;
    int rc = ensure_counts(c, 1);
    if (rc) return rc;
    const GridChoice ch = choose_grid_scale(s.scale, s.M, [&](const GridPlan &plan, long long nb, long long) {
        unsigned long long total = 0;
        rc = count_grid_entries(s, plan, nb, &total);
        return rc ? -1LL : (long long)std::min(total, 0x7fffffffffffffffull);
    });
    if (ch.result == GRID_SCALE_ABANDONED) return rc;
    if (ch.result != GRID_SCALE_OK) { c->last_error = "cell-lookup grid: no bucket size fits this mesh"; return MCRAT_HIP_EINVAL; }
    s.plan = ch.plan; s.nb = ch.nb; s.entries = ch.entries;
    if (getenv("MCRAT_HIP_VERBOSE"))
        fprintf(stderr, "mcrat_hip: cell-lookup grid %d x %d x %d buckets, %lld entries for %d cells (%.2f per bucket), built on the device\n",
                s.plan.dim[0], s.plan.dim[1], s.plan.dim[2], s.entries, s.M, (double)s.entries / (double)s.nb);
    return MCRAT_HIP_OK;
}

// (MCRAT_HIP_NO_COVERED in the environment: the grid without its covered-octant table, every lookup through the bucket records -- for A/B runs)
int ensure_grid_buffer(HydroStage &s)
{
    s.covered_ints = covered_table_ints(s.plan, s.nb, getenv("MCRAT_HIP_NO_COVERED") == nullptr);
    s.grid = grid_layout(s.nb, s.entries, grid_scan_scratch_ints(s.nb), s.covered_ints);
    if (getenv("MCRAT_HIP_VERBOSE"))
        fprintf(stderr, "mcrat_hip: covered-octant table %zu B of the grid's %zu B\n", s.grid.dir - s.grid.covered, s.grid.total);
    return ensure_device_bytes(s.c, &s.c->grid_buf, &s.c->grid_bytes, s.grid.total);
}

int build_grid_device(HydroStage &s)
{
    mcrat_hip_ctx *c = s.c;
    const GridLayout &g = s.grid;
    HIPCHK(c, grid_build(s.plan, c->hy.geom, c->hy.geom2, c->hy.fluid, c->hy.fluid_c, s.M, c->grid_count, s.grid_at<int>(g.start), s.grid_at<int>(g.scan),
                         s.grid_at<int>(g.entries), s.grid_at<FatCell>(g.cells), s.grid_at<BucketDir>(g.dir),
                         s.covered_ints ? s.grid_at<int>(g.covered) : nullptr, s.nb, s.entries, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

// host build: the bucket records and the lists -- complete copies of the member cells' records -- as the image of what the lookup reads, and up
int upload_host_grid(HydroStage &s, const HostFrame &hf)
{
    const GridHost &g = hf.grid;
    const CellGeom *geom = reinterpret_cast<const CellGeom *>(hf.image.data() + s.cells.geom);
    const CellFluid *fluid = reinterpret_cast<const CellFluid *>(hf.image.data() + s.cells.fluid);
    const bool three = s.cells.has_geom2;
    std::vector<char> gh(s.grid.start, 0);
    BucketDir *dir = reinterpret_cast<BucketDir *>(gh.data() + s.grid.dir);
    for (size_t b = 0; b < (size_t)s.nb; ++b) {
        dir[b].e0 = g.start[b]; dir[b].n = g.start[b + 1] - g.start[b]; dir[b].hints = g.hints[b]; dir[b].pad = 0;
    }
    if (s.covered_ints) memcpy(gh.data() + s.grid.covered, g.covered.data(), sizeof(int) * s.covered_ints);   // (the same size rule: build_grid)
    FatCell *fat = reinterpret_cast<FatCell *>(gh.data() + s.grid.cells);
    for (size_t e = 0; e < g.cells.size(); ++e) {
        const int ci = g.cells[e];
        fat[e] = fat_cell(geom[ci], fluid[ci], three ? hf.h->r2[ci] : 0.0, three ? hf.h->r2_size[ci] : 0.0, ci);
    }
    HIPCHK(s.c, hipMemcpy(s.c->grid_buf, gh.data(), s.grid.start, hipMemcpyHostToDevice));
    return MCRAT_HIP_OK;
}

void publish_grid(HydroStage &s)
{
    HydroDev &hy = s.c->hy;
    hy.grid.dir = s.grid_at<const BucketDir>(s.grid.dir);
    hy.grid.cells = s.grid_at<const FatCell>(s.grid.cells);
    grid_plan_to_dev(s.plan, hy.grid);
    hy.grid.cov_back = s.covered_ints ? (int)((s.grid.dir - s.grid.covered) / sizeof(int)) : 0;
    apply_hot_table(s.c);
}

// exp(x) K_2(x) of the hot cells, and the frame is there
int finish_frame(HydroStage &s)
{
    mcrat_hip_ctx *c = s.c;
    if (s.any_hot) {
        HIPCHK(c, launch_k2e(c->hy.temp, s.cell_at<double>(s.cells.k2e), s.M, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->have_hydro = true;
    drop_graph(c);
    sync_views(c);
    return MCRAT_HIP_OK;
}

}  // namespace

// the product path: everything on the device, from the columns in c->hcol
static int stage_hydro_device(HydroStage &s, const double *dom0, const double *dom1, const double *dom2)
{
    int rc;
    if ((rc = ensure_cell_buffer(s, true))) return rc;          // whether a cell is hot is known only after the staging: k2e is always reserved
    if ((rc = stage_cells_device(s))) return rc;
    publish_cells(s, dom0, dom1, dom2);
    if ((rc = choose_scale_device(s))) return rc;
    if ((rc = ensure_grid_buffer(s))) return rc;
    if ((rc = build_grid_device(s))) return rc;
    publish_grid(s);
    return finish_frame(s);
}
// the cross-check (MCRAT_HIP_HOST_GRID=1): staging loop and grid build on the host, from the caller's columns h
static int stage_hydro_host(HydroStage &s, const mcrat_hip_hydro *h, const double *dom0, const double *dom1, const double *dom2)
{
    HostFrame hf{h};
    int rc;
    if ((rc = host_build_grid(s, hf))) return rc;
    if ((rc = ensure_cell_buffer(s, s.any_hot))) return rc;
    if ((rc = stage_cells_host(s, hf))) return rc;
    publish_cells(s, dom0, dom1, dom2);
    if ((rc = ensure_grid_buffer(s))) return rc;
    if ((rc = upload_host_grid(s, hf))) return rc;
    publish_grid(s);
    return finish_frame(s);
}
static int stage_hydro(mcrat_hip_ctx *c, const mcrat_hip_hydro *h, int M, const double *dom0, const double *dom1, const double *dom2)
{
    if (c->hydro_owner) { c->last_error = "stage_hydro on a context that reads another one's frame"; return MCRAT_HIP_ESTATE; }   // (ensure_hcol released it)
    HydroStage s{c, M, c->kc.dimensions == DIM_THREE ? 3 : 2};
    return h ? stage_hydro_host(s, h, dom0, dom1, dom2) : stage_hydro_device(s, dom0, dom1, dom2);
}

// a context that reads another one's staged frame (mcrat_hip_share_hydro) holds that context's pointers: forget them before staging its own
static void release_shared_hydro(mcrat_hip_ctx *c)
{
    std::lock_guard<std::mutex> lock(g_share_mutex);
    if (!c->hydro_owner) return;
    auto &v = c->hydro_owner->hydro_sharers;
    v.erase(std::remove(v.begin(), v.end(), c), v.end());
    forget_shared_frame(c);
}

// Several contexts on one GPU that are in the same hydro frame (rank pools on their own streams, bench.py --pools) need
// one copy of the frame, its per-cell records and its lookup grid, not one each: `ctx` reads `owner`'s staged frame (and cross-section table)
// from now on.  The owner must keep that frame (not re-stage, not be destroyed) while others read it; staging a frame on `ctx` itself, or
// sharing again, ends the arrangement.  Both contexts must be of the same DIMENSIONS / GEOMETRY / TAU_CALCULATION on the same device.
extern "C" int mcrat_hip_share_hydro(mcrat_hip_ctx *c, mcrat_hip_ctx *owner)
{
    if (!c || !owner || c == owner) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "share_hydro");
    if (owner->parent) owner = owner->parent;
    if (!owner->have_hydro || owner->hydro_owner == c) return MCRAT_HIP_ESTATE;
    if (owner->hydro_owner) owner = owner->hydro_owner;
    if (c->kc.dimensions != owner->kc.dimensions || c->kc.geometry != owner->kc.geometry || c->kc.table != owner->kc.table ||
        c->cfg.device != owner->cfg.device) {
        c->last_error = "share_hydro: the two contexts differ in DIMENSIONS / GEOMETRY / TAU_CALCULATION or device";
        return MCRAT_HIP_EINVAL;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(owner->stream));            // the owner's staging kernels have finished
    release_shared_hydro(c);
    detach_sharers(c, "shares another context's frame now");   // its own buffers go
    if (c->hy_buf) { HIPCHK(c, hipFree(c->hy_buf)); c->hy_buf = nullptr; c->hy_bytes = 0; }
    if (c->grid_buf) { HIPCHK(c, hipFree(c->grid_buf)); c->grid_buf = nullptr; c->grid_bytes = 0; }
    if (c->hcol_buf) { HIPCHK(c, hipFree(c->hcol_buf)); c->hcol_buf = nullptr; c->hcol_bytes = 0; }
    if (c->d_hot_table) { HIPCHK(c, hipFree(c->d_hot_table)); c->d_hot_table = nullptr; }
    c->hy = owner->hy;
    c->hcol = owner->hcol; c->hcol_buf = owner->hcol_buf; c->hcol_M = owner->hcol_M;
    c->d_hot_table = owner->d_hot_table; c->hot_n_ph_e = owner->hot_n_ph_e; c->hot_n_t = owner->hot_n_t;
    for (int k = 0; k < 4; ++k) c->hot_grid[k] = owner->hot_grid[k];
    apply_hot_table(c);                                        // (the count of lookups outside the table stays this context's own)
    c->have_hydro = true;
    {
        std::lock_guard<std::mutex> lock(g_share_mutex);
        c->hydro_owner = owner;
        owner->hydro_sharers.push_back(c);
    }
    c->frame_open = false;
    drop_graph(c);
    sync_views(c);
    return MCRAT_HIP_OK;
}

// struct hydro_dataframe's columns on the device: 16 arrays of M doubles
static int ensure_hcol(mcrat_hip_ctx *c, int M)
{
    release_shared_hydro(c);
    detach_sharers(c, "staged another frame");              // the buffers they point into are about to be rewritten or freed
    const size_t stride = align_up(sizeof(double) * (size_t)M, 256), total = 19 * stride;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    { int rc = ensure_device_bytes(c, &c->hcol_buf, &c->hcol_bytes, total); if (rc) return rc; }
    char *b = static_cast<char *>(c->hcol_buf);
    double **cols[19] = {&c->hcol.r0, &c->hcol.r1, &c->hcol.r2, &c->hcol.s0, &c->hcol.s1, &c->hcol.s2, &c->hcol.v0, &c->hcol.v1, &c->hcol.v2,
                         &c->hcol.dens, &c->hcol.dens_lab, &c->hcol.pres, &c->hcol.temp, &c->hcol.gamma, &c->hcol.r, &c->hcol.theta,
                         &c->hcol.B0, &c->hcol.B1, &c->hcol.B2};
    for (int k = 0; k < 19; ++k) *cols[k] = reinterpret_cast<double *>(b + k * stride);
    c->hcol_M = M;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_set_hydro(mcrat_hip_ctx *c, const mcrat_hip_hydro *h)
{
    if (!c || !h || h->num_elements <= 0) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "set_hydro");
    const int M = h->num_elements;
    const bool three = c->kc.dimensions == DIM_THREE, two = c->kc.dimensions == DIM_TWO;
    if (!h->r0 || !h->r1 || !h->r0_size || !h->r1_size || !h->v0 || !h->v1 || !h->dens_lab || !h->temp || !h->gamma) return MCRAT_HIP_EINVAL;
    if (three && (!h->r2 || !h->r2_size)) return MCRAT_HIP_EINVAL;
    if (!two && !h->v2) return MCRAT_HIP_EINVAL;
    c->have_hydro = false;
    sync_views(c);
    // the columns cross PCIe as they lie in the caller's memory; per-cell records and the cell-lookup grid are produced on
    // the device (stage_hydro)
    int rc = ensure_hcol(c, M);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->hcol_buf, 0, c->hcol_bytes, c->stream));
    const struct { double *dst; const double *src; } copy[12] = {
        {c->hcol.r0, h->r0}, {c->hcol.r1, h->r1}, {c->hcol.r2, three ? h->r2 : nullptr}, {c->hcol.s0, h->r0_size}, {c->hcol.s1, h->r1_size},
        {c->hcol.s2, three ? h->r2_size : nullptr}, {c->hcol.v0, h->v0}, {c->hcol.v1, h->v1}, {c->hcol.v2, !two ? h->v2 : nullptr},
        {c->hcol.dens_lab, h->dens_lab}, {c->hcol.temp, h->temp}, {c->hcol.gamma, h->gamma}};
    for (const auto &cp : copy)
        if (cp.src) HIPCHK(c, hipMemcpyAsync(cp.dst, cp.src, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_fill_spherical(c->kc.dimensions, c->kc.geometry, c->hcol, M, c->stream));
    return stage_hydro(c, getenv("MCRAT_HIP_HOST_GRID") ? h : nullptr, M, h->r0_domain, h->r1_domain, h->r2_domain);
}

extern "C" void mcrat_hip_outflow_defaults(int simulation_type, mcrat_hip_outflow *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->simulation_type = simulation_type;
    if (simulation_type == MCRAT_HIP_CYLINDRICAL_OUTFLOW) { o->gamma_infinity = 100; o->t_comov = 1e5; o->ddensity = 3e-7; }                      // analytic_outflows.c:5
    if (simulation_type == MCRAT_HIP_SPHERICAL_OUTFLOW) { o->gamma_infinity = 100; o->lumi = 1e54; o->r00 = 1e8; }                                // :65
    if (simulation_type == MCRAT_HIP_STRUCTURED_SPHERICAL_OUTFLOW) { o->gamma_infinity = 100; o->lumi = 1e52; o->r00 = 1e8; o->theta_j = 1e-2; o->p = 4; }   // :140
}

namespace {

// device copies of a reader's buffers, packed into c->raw_buf
struct RawPacker {
    mcrat_hip_ctx *c;
    size_t off = 0;
    std::vector<std::pair<size_t, std::pair<const void *, size_t>>> items;
    size_t add(const void *src, size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); items.push_back({o, {src, bytes}}); return o; }
    int upload()
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        { int rc = ensure_device_bytes(c, &c->raw_buf, &c->raw_bytes, off); if (rc) return rc; }
        for (const auto &it : items)
            if (it.second.first) HIPCHK(c, hipMemcpyAsync(static_cast<char *>(c->raw_buf) + it.first, it.second.first, it.second.second, hipMemcpyHostToDevice, c->stream));
        return MCRAT_HIP_OK;
    }
    template <class T> const T *at(size_t o) const { return reinterpret_cast<const T *>(static_cast<const char *>(c->raw_buf) + o); }
};

// the part of getHydroData both readers share: count with a growing elem_factor, scan, write, fill r/theta, overwrite
// with the analytic outflow, stage
template <class Count, class Write>
int ingest_common(mcrat_hip_ctx *c, long long n_virtual, const mcrat_hip_slab *slab, const mcrat_hip_outflow *outflow,
                  mcrat_hip_ingest_result *result, Count count, Write write)
{
    const long long nblk = ingest_blocks(n_virtual);
    if (nblk <= 0 || nblk > 0x7fffffffLL) return MCRAT_HIP_EINVAL;
    { int rc_ = ensure_counts(c, (size_t)nblk); if (rc_) return rc_; }
    // CYCLOSYNCHROTRON_SWITCH is OFF in this engine (mcrat_hip_init refuses it): elem_factor starts at 0 (mclib_flash.c:275-279)
    int elem_factor = 0;
    unsigned long long total = 0;
    SlabDev sd{};
    while (total == 0) {
        elem_factor++;
        if (elem_factor > 1000) {
            c->last_error = "hydro ingest: no cell lies in the requested slab for any elem_factor up to 1000 (the reference would not return)";
            return MCRAT_HIP_EINVAL;
        }
        sd = slab_for(c->kc.dimensions, c->kc.geometry, slab, elem_factor);
        HIPCHK(c, count(sd));
        HIPCHK(c, hipMemcpyAsync(&total, c->d_grid_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (total > 0x7fffffffull) { c->last_error = "hydro ingest: more than INT_MAX cells selected"; return MCRAT_HIP_EINVAL; }
    const int M = (int)total;
    int rc = ensure_hcol(c, M);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->hcol_buf, 0, c->hcol_bytes, c->stream));
    const size_t scan_bytes = sizeof(int) * ((size_t)nblk + 1 + grid_scan_scratch_ints(nblk));
    if ((rc = ensure_aos(c, scan_bytes))) return rc;
    int *start = static_cast<int *>(c->aos_buf), *scratch = start + nblk + 1;
    HIPCHK(c, launch_exclusive_scan(c->grid_count, nblk, start, scratch, (long long)total, c->stream));
    HIPCHK(c, write(sd, start));
    HIPCHK(c, launch_fill_spherical(c->kc.dimensions, c->kc.geometry, c->hcol, M, c->stream));          // mcrat_io.c:1962
    if (outflow && outflow->simulation_type != MCRAT_HIP_SCIENCE) {                                      // mcrat_io.c:1967-1973
        OutflowDev o{outflow->simulation_type, outflow->gamma_infinity, outflow->lumi, outflow->r00, outflow->t_comov, outflow->ddensity,
                     outflow->theta_j, outflow->p};
        HIPCHK(c, launch_outflow_prep(c->kc.dimensions, c->kc.geometry, o, c->hcol, M, c->stream));
    }
    if (result) { result->num_elements = M; result->elem_factor = elem_factor; }
    return stage_hydro(c, nullptr, M, slab->r0_domain, slab->r1_domain, slab->r2_domain);
}

}  // namespace

extern "C" int mcrat_hip_ingest_flash(mcrat_hip_ctx *c, const mcrat_hip_flash_blocks *b, const mcrat_hip_slab *slab, const mcrat_hip_outflow *outflow,
                                      mcrat_hip_ingest_result *result)
{
    if (!c || !b || !slab_ok(slab) || !outflow_ok(outflow)) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "ingest_flash");
    if (b->n_blocks <= 0 || b->coord_stride < 2 || b->bsize_stride < 2 || !b->coordinates || !b->block_size || !b->node_type || !b->velx || !b->vely ||
        !b->dens || !b->pres)
        return MCRAT_HIP_EINVAL;
    if (c->kc.dimensions != DIM_TWO) { c->last_error = "FLASH frames are two-dimensional (mcrat_io.c:1938: 3D FLASH is not supported)"; return MCRAT_HIP_EINVAL; }
    c->have_hydro = false;
    sync_views(c);
    const size_t nb = (size_t)b->n_blocks;
    RawPacker pk{c};
    const size_t o_coord = pk.add(b->coordinates, sizeof(double) * nb * b->coord_stride), o_bs = pk.add(b->block_size, sizeof(double) * nb * b->bsize_stride);
    const size_t o_node = pk.add(b->node_type, sizeof(int) * nb);
    const size_t o_vx = pk.add(b->velx, sizeof(double) * nb * 64), o_vy = pk.add(b->vely, sizeof(double) * nb * 64);
    const size_t o_d = pk.add(b->dens, sizeof(double) * nb * 64), o_p = pk.add(b->pres, sizeof(double) * nb * 64);
    int rc = pk.upload();
    if (rc) return rc;
    FlashDev f{};
    f.coord = pk.at<double>(o_coord); f.bsize = pk.at<double>(o_bs); f.node = pk.at<int>(o_node);
    f.velx = pk.at<double>(o_vx); f.vely = pk.at<double>(o_vy); f.dens = pk.at<double>(o_d); f.pres = pk.at<double>(o_p);
    f.coord_stride = b->coord_stride; f.bsize_stride = b->bsize_stride; f.n_blocks = b->n_blocks;
    f.L = b->l_scale; f.D = b->d_scale; f.P = b->p_scale;
    if (result) { memset(result, 0, sizeof *result); }
    rc = ingest_common(c, (long long)nb * 64, slab, outflow, result,
                       [&](const SlabDev &sd) { return ingest_count_flash(f, sd, c->grid_count, c->d_grid_total, c->stream); },
                       [&](const SlabDev &sd, const int *start) { return ingest_write_flash(f, sd, start, c->hcol, c->stream); });
    if (rc == MCRAT_HIP_OK && result) {
        long long leaves = 0;
        for (size_t i = 0; i < nb; ++i) leaves += b->node_type[i] == 1;
        result->cells_read = leaves * 64;
    }
    return rc;
}

extern "C" int mcrat_hip_ingest_pluto(mcrat_hip_ctx *c, const mcrat_hip_pluto_grid *g, const mcrat_hip_slab *slab, const mcrat_hip_outflow *outflow,
                                      mcrat_hip_ingest_result *result)
{
    if (!c || !g || !slab_ok(slab) || !outflow_ok(outflow)) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "ingest_pluto");
    const bool three = c->kc.dimensions == DIM_THREE, two = c->kc.dimensions == DIM_TWO;
    if (g->nx <= 0 || g->ny <= 0 || (three && g->nz <= 0) || !g->x1 || !g->dx1 || !g->x2 || !g->dx2 || !g->rho || !g->vx1 || !g->vx2 || !g->prs)
        return MCRAT_HIP_EINVAL;
    if (three && (!g->x3 || !g->dx3)) return MCRAT_HIP_EINVAL;
    if (!two && !g->vx3) return MCRAT_HIP_EINVAL;
    const int nz = three ? g->nz : 1;
    const size_t cells = (size_t)g->nx * g->ny * nz;
    if (cells > 0x7fffffffull) return MCRAT_HIP_EINVAL;            // the reference's grid_size is an int (mclib_pluto.c:1061)
    c->have_hydro = false;
    sync_views(c);
    RawPacker pk{c};
    const size_t o_x1 = pk.add(g->x1, sizeof(double) * g->nx), o_dx1 = pk.add(g->dx1, sizeof(double) * g->nx);
    const size_t o_x2 = pk.add(g->x2, sizeof(double) * g->ny), o_dx2 = pk.add(g->dx2, sizeof(double) * g->ny);
    const size_t o_x3 = three ? pk.add(g->x3, sizeof(double) * nz) : 0, o_dx3 = three ? pk.add(g->dx3, sizeof(double) * nz) : 0;
    const size_t o_rho = pk.add(g->rho, sizeof(double) * cells), o_v1 = pk.add(g->vx1, sizeof(double) * cells), o_v2 = pk.add(g->vx2, sizeof(double) * cells);
    const size_t o_v3 = !two ? pk.add(g->vx3, sizeof(double) * cells) : 0, o_p = pk.add(g->prs, sizeof(double) * cells);
    int rc = pk.upload();
    if (rc) return rc;
    PlutoDev d{};
    d.nx = g->nx; d.ny = g->ny; d.nz = nz;
    d.x1 = pk.at<double>(o_x1); d.dx1 = pk.at<double>(o_dx1); d.x2 = pk.at<double>(o_x2); d.dx2 = pk.at<double>(o_dx2);
    d.x3 = three ? pk.at<double>(o_x3) : nullptr; d.dx3 = three ? pk.at<double>(o_dx3) : nullptr;
    d.rho = pk.at<double>(o_rho); d.vx1 = pk.at<double>(o_v1); d.vx2 = pk.at<double>(o_v2); d.vx3 = !two ? pk.at<double>(o_v3) : nullptr;
    d.prs = pk.at<double>(o_p);
    d.L = g->l_scale; d.D = g->d_scale; d.P = g->p_scale;
    if (result) { memset(result, 0, sizeof *result); }
    rc = ingest_common(c, (long long)cells, slab, outflow, result,
                       [&](const SlabDev &sd) { return ingest_count_pluto(d, sd, c->grid_count, c->d_grid_total, c->stream); },
                       [&](const SlabDev &sd, const int *start) { return ingest_write_pluto(d, sd, start, c->hcol, c->stream); });
    if (rc == MCRAT_HIP_OK && result) result->cells_read = (long long)cells;
    return rc;
}

extern "C" int mcrat_hip_ingest_chombo(mcrat_hip_ctx *c, const mcrat_hip_chombo *h, const mcrat_hip_slab *slab, const mcrat_hip_outflow *outflow,
                                       mcrat_hip_ingest_result *result)
{
    if (!c || !h || !slab_ok(slab) || !outflow_ok(outflow)) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "ingest_chombo");
    if (h->num_levels <= 0 || h->num_vars <= 0 || !h->levels || !h->var_names || !h->data) return MCRAT_HIP_EINVAL;
    const bool three = c->kc.dimensions == DIM_THREE;
    const int nd = three ? 3 : 2, nl = h->num_levels;
    ChomboPlan plan;                                             // the box table and the per-level coordinate arrays (hydro_plan.hpp)
    if (const char *why = chombo_plan(h, c->kc.dimensions, plan)) {
        if (*why) c->last_error = why;
        return MCRAT_HIP_EINVAL;
    }
    const std::vector<ChomboBox> &boxes = plan.boxes;
    const std::vector<int> &level_first_box = plan.level_first_box;
    const long long total = plan.total, cells = plan.cells;

    c->have_hydro = false;
    sync_views(c);
    const bool masked = slab->ph_inj_switch != 0;
    RawPacker pk{c};
    const size_t o_box = pk.add(boxes.data(), sizeof(ChomboBox) * boxes.size());
    size_t o_x[3] = {0, 0, 0}, o_dx[3] = {0, 0, 0};
    for (int a = 0; a < nd; ++a) { o_x[a] = pk.add(plan.xs[a].data(), sizeof(double) * plan.xs[a].size()); o_dx[a] = pk.add(plan.dxs[a].data(), sizeof(double) * plan.dxs[a].size()); }
    const size_t o_data = pk.add(h->data, sizeof(double) * (size_t)total);
    const size_t o_mask = masked ? pk.add(nullptr, (size_t)cells) : 0;
    int rc = pk.upload();
    if (rc) return rc;
    ChomboDev d{};
    d.boxes = pk.at<ChomboBox>(o_box); d.n_boxes = (int)boxes.size(); d.cells = cells;
    d.data = pk.at<double>(o_data);
    for (int a = 0; a < nd; ++a) { d.x[a] = pk.at<double>(o_x[a]); d.dx[a] = pk.at<double>(o_dx[a]); }
    for (int w = 0; w < 5; ++w) d.kv[w] = plan.kv[w];
    d.L = h->l_scale; d.D = h->d_scale; d.P = h->p_scale;
    if (masked) {
        unsigned char *mask = static_cast<unsigned char *>(c->raw_buf) + o_mask;
        HIPCHK(c, hipMemsetAsync(mask, 0, (size_t)cells, c->stream));
        for (int i = nl - 2; i >= 0; --i)                      // :206-345
            HIPCHK(c, launch_chombo_mask(d.boxes, level_first_box[i], level_first_box[i + 1], level_first_box[i + 1], level_first_box[i + 2],
                                         h->levels[i].ref_ratio, three ? 1 : 0, mask, c->stream));
        d.covered = mask;
    }
    if (result) { memset(result, 0, sizeof *result); }
    rc = ingest_common(c, cells, slab, outflow, result,
                       [&](const SlabDev &sd) { return ingest_count_chombo(d, sd, c->grid_count, c->d_grid_total, c->stream); },
                       [&](const SlabDev &sd, const int *start) { return ingest_write_chombo(d, sd, start, c->hcol, c->stream); });
    if (rc == MCRAT_HIP_OK && result) result->cells_read = cells;
    return rc;
}

extern "C" int mcrat_hip_set_hydro_extras(mcrat_hip_ctx *c, const double *dens, const double *B0, const double *B1, const double *B2)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->parent) return view_refuses(c, "set_hydro_extras");
    if (!c->have_hydro || !c->hcol_buf) return MCRAT_HIP_ESTATE;
    const size_t bytes = sizeof(double) * (size_t)c->hcol_M;
    const struct { double *dst; const double *src; } copy[4] = {{c->hcol.dens, dens}, {c->hcol.B0, B0}, {c->hcol.B1, B1}, {c->hcol.B2, B2}};
    for (const auto &cp : copy)
        if (cp.src) HIPCHK(c, hipMemcpyAsync(cp.dst, cp.src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_absorb_cyclosynch(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, int *num_abs_ph, int *scatt_cyclosynch_num_ph,
                                           double *abs_weight)
{
    if (!c || !cs || cs->b_field_calc < 0 || cs->b_field_calc > 2) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro || !c->have_photons || !c->hcol_buf) return MCRAT_HIP_ESTATE;
    int rc = flush_pending(c);
    if (rc) return rc;
    const int nblk = cs_absorb_blocks(c->ph.n);
    if ((rc = ensure_aos(c, sizeof(CsAbsPartial) * (size_t)nblk))) return rc;
    CsParams p{c->kc.dimensions, cs->b_field_calc, cs->epsilon_b};
    HIPCHK(c, launch_cs_absorb(p, c->ph, c->hy.temp, c->hcol, static_cast<CsAbsPartial *>(c->aos_buf), c->stream));
    std::vector<CsAbsPartial> part((size_t)nblk);
    HIPCHK(c, hipMemcpyAsync(part.data(), c->aos_buf, sizeof(CsAbsPartial) * (size_t)nblk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double w = 0;
    long long a = 0, s = 0;
    for (const auto &q : part) { w += q.abs_weight; a += q.abs_count; s += q.scatt_count; }
    if (num_abs_ph) *num_abs_ph = (int)a;
    if (scatt_cyclosynch_num_ph) *scatt_cyclosynch_num_ph = (int)s;
    if (abs_weight) *abs_weight = w;
    drop_graph(c);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_get_hydro(mcrat_hip_ctx *c, mcrat_hip_hydro_columns *out)
{
    if (!c || !out) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro || !c->hcol_buf) return MCRAT_HIP_ESTATE;
    const int M = c->hcol_M;
    if (out->num_elements < M) return MCRAT_HIP_EINVAL;
    const struct { double *dst; const double *src; } copy[16] = {
        {out->r0, c->hcol.r0}, {out->r1, c->hcol.r1}, {out->r2, c->hcol.r2}, {out->r0_size, c->hcol.s0}, {out->r1_size, c->hcol.s1},
        {out->r2_size, c->hcol.s2}, {out->v0, c->hcol.v0}, {out->v1, c->hcol.v1}, {out->v2, c->hcol.v2}, {out->dens, c->hcol.dens},
        {out->dens_lab, c->hcol.dens_lab}, {out->pres, c->hcol.pres}, {out->temp, c->hcol.temp}, {out->gamma, c->hcol.gamma},
        {out->r, c->hcol.r}, {out->theta, c->hcol.theta}};
    for (const auto &cp : copy)
        if (cp.dst) HIPCHK(c, hipMemcpyAsync(cp.dst, cp.src, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->num_elements = M;
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- photons
// a view's list: a window of `n` slots into the pool's columns (the window spans the pool's slots per rank; slots beyond n stay invalid)
static int alloc_view_photons(mcrat_hip_ctx *c, int n, bool clear_window = true)
{
    mcrat_hip_ctx *P = c->parent;
    if (n > P->rank_stride) {
        c->last_error = "the list is longer than the pool's slots per rank (mcrat_hip_pool_create)";
        return MCRAT_HIP_ENOMEM;
    }
    c->ph = photon_window(P->ph, c->view_rank, P->rank_stride, n);
    if (clear_window) HIPCHK(c, launch_clear_slots(c->ph, 0, P->rank_stride, c->stream));
    c->step_blocks = step_grid_blocks(c->ph.n_pad);
    c->partials = P->partials;                // list-mode scratch is the pool's: one stream, one list at a time
    c->partials_bytes = P->partials_bytes;
    c->shortlist = P->shortlist;
    if (clear_window) HIPCHK(c, hipMemsetAsync(c->shortlist, 0, sizeof(Shortlist), c->stream));
    c->n_ranks = 0;
    drop_graph(c);
    return MCRAT_HIP_OK;
}

static int alloc_photons(mcrat_hip_ctx *c, int n)
{
    if (c->parent) return alloc_view_photons(c, n);
    if (c->is_pool) {
        c->last_error = "this context is a rank pool: its photons are set through the views (mcrat_hip_pool_rank)";
        return MCRAT_HIP_ESTATE;
    }
    int rc;
    // the layout
    if (const PhotonLayoutStatus why = photon_layout(n, &c->ph_lay)) { c->last_error = photon_layout_text(why); return MCRAT_HIP_EINVAL; }
    // the buffer, zeroed
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = ensure_device_bytes(c, &c->ph_buf, &c->ph_bytes, c->ph_lay.total))) return rc;
    HIPCHK(c, hipMemsetAsync(c->ph_buf, 0, c->ph_lay.total, c->stream));
    // the columns
    c->ph = bind_photons(c->ph_lay, c->ph_buf, n);
    // the context's scratch: one candidate per workgroup of the step kernel, one LoopState per virtual rank, the shortlist
    c->step_blocks = step_grid_blocks(c->ph.n_pad);
    if ((rc = ensure_device_bytes(c, (void **)&c->partials, &c->partials_bytes, sizeof(Cand) * (size_t)c->step_blocks))) return rc;
    c->n_ranks = 0;
    if (c->cfg.virtual_rank_photons > 0) {
        c->rank_stride = c->cfg.virtual_rank_photons;
        c->n_ranks = (n + c->cfg.virtual_rank_photons - 1) / c->cfg.virtual_rank_photons;
        const size_t bytes = sizeof(LoopState) * (size_t)c->n_ranks;
        if ((rc = ensure_device_bytes(c, (void **)&c->d_rstates, &c->d_rstates_bytes, bytes))) return rc;
        if ((rc = ensure_host_bytes(c, (void **)&c->h_rstates, &c->h_rstates_bytes, bytes))) return rc;
    }
    if (!c->shortlist) HIPCHK(c, hipMalloc((void **)&c->shortlist, sizeof(Shortlist)));
    HIPCHK(c, hipMemsetAsync(c->shortlist, 0, sizeof(Shortlist), c->stream));
    drop_graph(c);
    return MCRAT_HIP_OK;
}

// a list has come in: the context holds photons, and whatever frame was open is not theirs
static void photons_are_set(mcrat_hip_ctx *c) { c->have_photons = true; c->frame_open = false; }

// the caller's columns into the list's, with the derived columns and the flag byte made from them (photon_plan.hpp)
static int upload_columns(mcrat_hip_ctx *c, const mcrat_hip_photon_soa *s)
{
    const PhotonDev &p = c->ph;
    const size_t n = (size_t)s->n;
    for (int k = 0; k < N_ABI_COLS; ++k)
        if (s->*SOA_COLS[k]) HIPCHK(c, hipMemcpyAsync(p.*PHOTON_COLS[k], s->*SOA_COLS[k], sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    std::vector<double> der(4 * n);
    derived_columns(s->n, s->p0, s->p1, s->p2, s->p3, s->total_optical_depth, der.data());
    double *const derived[4] = {p.u0, p.u1, p.u2, p.ntau};
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(derived[k], der.data() + k * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    std::vector<unsigned char> flags(n);
    for (size_t i = 0; i < n; ++i) flags[i] = make_flags(s->type[i], s->weight[i], s->recalc_properties[i]);
    HIPCHK(c, hipMemcpyAsync(p.idx, s->nearest_block_index, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.flags, flags.data(), n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.type, s->type, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    photons_are_set(c);
    return MCRAT_HIP_OK;
}

static int ensure_aos(mcrat_hip_ctx *c, size_t bytes)
{
    if (c->parent) {                               // a view borrows its pool's staging buffer (ensure_counts)
        int rc = ensure_aos(c->parent, bytes);
        c->aos_buf = c->parent->aos_buf; c->aos_bytes = c->parent->aos_bytes;
        return rc;
    }
    return ensure_device_bytes(c, &c->aos_buf, &c->aos_bytes, bytes);
}

// Page-lock the caller's memory (its struct photon array, its hydro columns) so that the copies of set_photons / get_photons /
// set_hydro run as direct DMA at the link's rate instead of through the runtime's staging of pageable memory.
extern "C" int mcrat_hip_register_host(mcrat_hip_ctx *c, void *ptr, size_t bytes)
{
    if (!c || !ptr || bytes == 0) return MCRAT_HIP_EINVAL;
    HIPCHK(c, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_unregister_host(mcrat_hip_ctx *c, void *ptr)
{
    if (!c || !ptr) return MCRAT_HIP_EINVAL;
    HIPCHK(c, hipHostUnregister(ptr));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_set_photons(mcrat_hip_ctx *c, const mcrat_hip_photon_list *l)
{
    if (!c || !l || !l->photons || l->list_capacity <= 0) return MCRAT_HIP_EINVAL;
    const int n = l->list_capacity;
    int rc = alloc_photons(c, n);
    if (rc) return rc;
    // the records cross PCIe as they lie in the caller's memory; staging.hip transposes them on the device
    const size_t bytes = sizeof(mcrat_hip_photon) * (size_t)n;
    if ((rc = ensure_aos(c, bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->aos_buf, l->photons, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_aos_to_soa(c->aos_buf, c->ph, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    photons_are_set(c);
    return MCRAT_HIP_OK;
}

// mcrat_hip_set_photons for many lists of a rank pool at once (a CONTINUE run's restart: every adopted rank's checkpoint, mcrat.c:235-330 /
// readCheckpoint): the lists' records are gathered into one staging buffer, cross PCIe in ONE copy and are transposed into their windows by ONE
// launch, instead of a copy, two launches and a wait per list.  rank_of[j] is the pool rank list j goes to (its view must exist:
// mcrat_hip_pool_rank); every list exactly as mcrat_hip_set_photons(view, list) would leave it.
extern "C" int mcrat_hip_pool_set_photons(mcrat_hip_ctx *c, int count, const int *rank_of, const mcrat_hip_photon_list *lists)
{
    if (!c || count < 0 || (count > 0 && (!rank_of || !lists))) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "pool_set_photons")) return rc_;
    if (count == 0) return MCRAT_HIP_OK;
    struct Desc { int rank, n; long long first; };
    static_assert(sizeof(Desc) == 16, "PoolSetDesc of staging.hip");
    std::vector<Desc> desc((size_t)count);
    std::vector<char> seen((size_t)c->n_ranks, 0);
    size_t total = 0;
    for (int j = 0; j < count; ++j) {                                       // everything is checked before any window is touched
        const int r = rank_of[j];
        if (r < 0 || r >= c->n_ranks || !lists[j].photons || lists[j].list_capacity <= 0 || seen[(size_t)r]) return MCRAT_HIP_EINVAL;
        seen[(size_t)r] = 1;
        if (!c->views[r]) { c->last_error = "pool_set_photons: a list without a view (mcrat_hip_pool_rank)"; return MCRAT_HIP_ESTATE; }
        if (lists[j].list_capacity > c->rank_stride) { c->last_error = "a list is longer than the pool's slots per rank (mcrat_hip_pool_create)"; return MCRAT_HIP_ENOMEM; }
        desc[(size_t)j] = Desc{r, lists[j].list_capacity, (long long)total};
        total += (size_t)lists[j].list_capacity;
    }
    const size_t rec_bytes = sizeof(mcrat_hip_photon) * total, desc_bytes = sizeof(Desc) * (size_t)count;
    int rc = ensure_aos(c, align_up(rec_bytes, 256) + desc_bytes);
    if (rc) return rc;
    char *dev = static_cast<char *>(c->aos_buf);
    {   // the lists' records, gathered through two pinned pieces: the copy into one overlaps the transfer of the other (a pageable source
        // of this size moves at 3 GB/s; the caller's lists are wherever readCheckpoint put them)
        constexpr size_t PIECE = 16u << 20;
        for (int k = 0; k < 2; ++k) {
            if (!c->pin_ring[k]) HIPCHK(c, hipHostMalloc(&c->pin_ring[k], PIECE, hipHostMallocDefault));
            if (!c->pin_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming));
        }
        size_t done = 0;            // bytes of the concatenated records already on their way
        int j = 0, k = 0;
        size_t in_list = 0;         // bytes of list j already taken
        bool used[2] = {false, false};
        while (done < rec_bytes) {
            if (used[k]) HIPCHK(c, hipEventSynchronize(c->pin_ev[k]));
            char *dst = static_cast<char *>(c->pin_ring[k]);
            size_t fill = 0;
            while (fill < PIECE && j < count) {
                const size_t list_bytes = sizeof(mcrat_hip_photon) * (size_t)lists[j].list_capacity;
                const size_t take = std::min(PIECE - fill, list_bytes - in_list);
                memcpy(dst + fill, reinterpret_cast<const char *>(lists[j].photons) + in_list, take);
                fill += take; in_list += take;
                if (in_list == list_bytes) { ++j; in_list = 0; }
            }
            HIPCHK(c, hipMemcpyAsync(dev + done, dst, fill, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipEventRecord(c->pin_ev[k], c->stream));
            used[k] = true;
            done += fill;
            k ^= 1;
        }
    }
    HIPCHK(c, hipMemcpyAsync(dev + align_up(rec_bytes, 256), desc.data(), desc_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_pool_aos_to_soa(dev, c->ph, c->rank_stride, dev + align_up(rec_bytes, 256), count, c->stream));
    for (int j = 0; j < count; ++j) {
        mcrat_hip_ctx *v = c->views[desc[(size_t)j].rank];
        if ((rc = alloc_view_photons(v, desc[(size_t)j].n, false))) { c->last_error = v->last_error; return rc; }    // the view's columns in place; the launch above filled and cleared the window
        photons_are_set(v);
    }
    HIPCHK(c, hipMemsetAsync(c->shortlist, 0, sizeof(Shortlist), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_inject_photons(mcrat_hip_ctx *c, double r_inj, double ph_weight, int min_photons, int max_photons, char spect,
                                        double theta_min, double theta_max, double fps, uint64_t seed, int *num_photons,
                                        double *ph_weight_adjusted)
{
    if (!c || !(ph_weight > 0) || !(fps > 0) || min_photons < 0 || max_photons < min_photons || (spect != 'b' && spect != 'w')) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    const int M = c->hy.M;
    const RadialRange slab = inject_slab_radii(r_inj, fps);
    const InjectParams p = inject_params(c, Region{slab.rmin, slab.rmax, theta_min, theta_max, spect == 'w'});
    RngKey key = c->key;
    key.seed = seed;
    { int rc_ = ensure_counts(c, (size_t)M); if (rc_) return rc_; }
    // mclib.c:87-136: draw the per-cell counts until the weight fits (weight_search_step)
    double weight = ph_weight;
    unsigned long long total = 0;
    bool ok = false;
    for (unsigned long long attempt = 0; attempt <= 200 && !ok; ++attempt) {
        HIPCHK(c, launch_birth_count(p, c->hy, weight, attempt, key, c->grid_count, c->d_grid_total, c->stream));
        HIPCHK(c, hipMemcpyAsync(&total, c->d_grid_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ok = weight_search_step(total, min_photons, (double)max_photons, &weight);
    }
    if (!ok) { c->last_error = list_refusal_text(INJECT_NO_WEIGHT); return MCRAT_HIP_EINVAL; }
    if (total == 0) { c->last_error = list_refusal_text(INJECT_NO_PHOTONS); return MCRAT_HIP_EINVAL; }
    const int n = (int)total;
    int rc = alloc_photons(c, n);
    if (rc) return rc;
    // cell -> first photon: exclusive scan of the counts (scratch: the record staging buffer)
    const size_t scan_bytes = sizeof(int) * ((size_t)M + 1 + grid_scan_scratch_ints(M));
    if ((rc = ensure_aos(c, scan_bytes))) return rc;
    int *start = static_cast<int *>(c->aos_buf), *scratch = start + M + 1;
    HIPCHK(c, launch_exclusive_scan(c->grid_count, M, start, scratch, (long long)total, c->stream));
    HIPCHK(c, launch_inject_generate(p, c->hy, weight, key, start, c->ph, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    photons_are_set(c);
    if (num_photons) *num_photons = n;
    if (ph_weight_adjusted) *ph_weight_adjusted = weight;
    return MCRAT_HIP_OK;
}

// photonInjection (mclib.c:9-300) for the lists of a rank pool that ask for it, a handful of launches for all of them: the injection slab
// of each group of lists that share one (same radius, angles and spectrum: the ranks of an angle bin) is found once, then one workgroup per
// list runs the list's weight loop and writes its photons into the list's window (inject.hip).  Every list gets exactly the photons
// mcrat_hip_inject_photons gives its view (same keys); a list with more photons than the kernel's table holds takes that path.
extern "C" int mcrat_hip_pool_inject_photons(mcrat_hip_ctx *c, double fps, mcrat_hip_pool_inject_list *lists)
{
    if (!c || !lists || !(fps > 0)) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "pool_inject_photons")) return rc_;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    const int R = c->n_ranks, M = c->hy.M;
    std::vector<Region> slabs((size_t)R);                   // the lists grouped by their slab
    int n_slabs = 0;
    std::vector<PoolInject> pi((size_t)R);
    bool any = false;
    int rc;
    // every list's arguments are looked at before any window is touched: a bad request for list 7 must not leave lists 0-6 emptied
    for (int r = 0; r < R; ++r) {
        mcrat_hip_pool_inject_list &q = lists[r];
        q.status = MCRAT_HIP_OK;
        if (!q.inject) continue;
        if (!(q.ph_weight > 0) || q.min_photons < 0 || q.max_photons < q.min_photons || (q.spect != 'b' && q.spect != 'w')) {
            q.status = MCRAT_HIP_EINVAL;
            c->last_error = "pool_inject_photons: a list's weight, photon-count range or spectrum is not valid";
            return MCRAT_HIP_EINVAL;
        }
        if (!c->views[r]) { q.status = MCRAT_HIP_ESTATE; c->last_error = "pool_inject_photons: a list without a view (mcrat_hip_pool_rank)"; return MCRAT_HIP_ESTATE; }
    }
    for (int r = 0; r < R; ++r) {
        pi[(size_t)r] = PoolInject{};
        mcrat_hip_pool_inject_list &q = lists[r];
        if (!q.inject) continue;
        mcrat_hip_ctx *v = c->views[r];
        if ((rc = alloc_view_photons(v, 0))) { c->last_error = v->last_error; return rc; }      // the window cleared, the view's columns in place
        v->have_photons = false;
        const RadialRange slab = inject_slab_radii(q.r_inj, fps);
        PoolInject &e = pi[(size_t)r];
        e.inject = 1; e.group = region_group(slabs.data(), &n_slabs, Region{slab.rmin, slab.rmax, q.theta_min, q.theta_max, q.spect == 'w'});
        e.seed = q.seed; e.stream = v->key.stream; e.weight_in = q.ph_weight; e.min_photons = q.min_photons; e.max_photons = q.max_photons;
        any = true;
    }
    if (!any) return MCRAT_HIP_OK;
    if ((rc = ensure_counts(c, (size_t)M + 8))) return rc;
    {                                                       // (the temporaries go before the lists are committed: a list may take the one-list path below)
        const size_t scan_ints = (size_t)M + 1 + grid_scan_scratch_ints(M);
        DeviceTemp<int> d_start;
        DeviceTemp<PoolInject> d_pi;
        DeviceTemp<InjectSlabCell> d_slab;
        if (d_start.alloc(scan_ints) != hipSuccess || d_pi.alloc((size_t)R) != hipSuccess) return MCRAT_HIP_ENOMEM;
        if (hipMemcpyAsync(d_pi, pi.data(), sizeof(PoolInject) * (size_t)R, hipMemcpyHostToDevice, c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
        for (int g = 0; g < n_slabs; ++g) {
            const InjectParams p = inject_params(c, slabs[(size_t)g]);
            int n_slab = 0;
            if ((rc = pool_region_cells(c, p, d_slab, &n_slab, [&] { return launch_region_write(p, c->hy, c->grid_count, n_slab, d_start, d_start + M + 1, d_slab, c->stream); })))
                return rc;
            if (launch_inject_pool(p, c->hy, c->ph, c->rank_stride, R, d_slab, n_slab, d_pi, g, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) { c->last_error = "photon injection of the pool's lists failed"; return MCRAT_HIP_EHIP; }
        }
        if (hipMemcpyAsync(pi.data(), d_pi, sizeof(PoolInject) * (size_t)R, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
    }
    // every list that was injected is committed; a list that failed says so in its own status (its window stays empty) and the call returns
    // the first such code after all lists have been looked at
    int first_error = MCRAT_HIP_OK;
    for (int r = 0; r < R; ++r) {
        const PoolInject &e = pi[(size_t)r];
        if (!e.inject) continue;
        mcrat_hip_ctx *v = c->views[r];
        mcrat_hip_pool_inject_list &q = lists[r];
        if (e.error == 3) {                                                 // more photons than the kernel's table: the one-list path (it says what is wrong, if anything)
            if ((rc = mcrat_hip_inject_photons(v, q.r_inj, q.ph_weight, q.min_photons, q.max_photons, q.spect, q.theta_min, q.theta_max, fps, q.seed,
                                               &q.num_photons, &q.ph_weight_adjusted))) {
                q.status = rc;
                if (!first_error) { first_error = rc; c->last_error = v->last_error; }
            }
            continue;
        }
        if (e.error == 1 || e.error == 2) {
            q.status = MCRAT_HIP_EINVAL; q.num_photons = 0;
            if (!first_error) {
                first_error = MCRAT_HIP_EINVAL;
                c->last_error = list_refusal_text(e.error == 1 ? INJECT_NO_WEIGHT : INJECT_NO_PHOTONS);
            }
            continue;
        }
        v->ph.n = e.n;
        photons_are_set(v);
        q.num_photons = e.n;
        q.ph_weight_adjusted = e.weight_out;
    }
    return first_error;
}

// reallocatePhotonListMemory (photons.c:37-80) on the device: a larger set of columns, the old slots copied, the new ones null
static int grow_photons(mcrat_hip_ctx *c, int new_n)
{
    const PhotonDev old = c->ph;
    void *old_buf = c->ph_buf;
    const int old_n = old.n;
    if (new_n <= old_n) return MCRAT_HIP_EINVAL;
    if (c->parent) {                                           // a view grows inside its window of the pool
        if (new_n > c->parent->rank_stride) {
            c->last_error = "the list cannot double: it would outgrow the pool's slots per rank (mcrat_hip_pool_create)";
            return MCRAT_HIP_ENOMEM;
        }
        HIPCHK(c, launch_null_fill(c->ph, old_n, new_n - old_n, c->stream));
        c->ph.n = new_n;
        return MCRAT_HIP_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // not the grow-only buffer as it is (ensure_device_bytes): a fresh, zeroed allocation, so that the old one is still there to be copied from
    const PhotonLayout old_lay = c->ph_lay;
    const size_t old_bytes = c->ph_bytes;
    c->ph_buf = nullptr; c->ph_bytes = 0;
    int rc = alloc_photons(c, new_n);
    if (rc) { if (c->ph_buf) (void)hipFree(c->ph_buf); c->ph_buf = old_buf; c->ph_bytes = old_bytes; c->ph_lay = old_lay; c->ph = old; return rc; }
    for (int k = 0; k < N_PHOTON_COLS; ++k)
        HIPCHK(c, hipMemcpyAsync(c->ph.*PHOTON_COLS[k], old.*PHOTON_COLS[k], sizeof(double) * (size_t)old_n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ph.idx, old.idx, sizeof(int) * (size_t)old_n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ph.flags, old.flags, (size_t)old_n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ph.type, old.type, (size_t)old_n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, launch_null_fill(c->ph, old_n, new_n - old_n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(old_buf));
    if (c->ph_snap) { HIPCHK(c, hipFree(c->ph_snap)); c->ph_snap = nullptr; c->ph_snap_bytes = 0; }     // a snapshot of the smaller list
    return MCRAT_HIP_OK;
}

// gsl_integration_qags (:1276) ran past the device's interval limit in `cells` cells (inject.hip, qags_planck): refused, and why
static int emit_not_converged(mcrat_hip_ctx *c, unsigned cells)
{
    char text[192];
    return c->last_error = emit_not_converged_text(text, sizeof text, cells), MCRAT_HIP_EREFUSED;
}

// The list's null slots in ascending order (addToPhotonList's null_ph_indexes, photons.c:181-189), in two halves because the host has to know
// their number before it can give them room.  First the count per 256 slots into block_count[0 .. (n + 255) / 256), its total on its way to
// *n_null: good once the caller has waited for the stream ...
static int null_slots_count(mcrat_hip_ctx *c, unsigned *block_count, unsigned long long *n_null)
{
    HIPCHK(c, launch_null_count(c->ph, block_count, c->d_grid_total, c->stream));
    HIPCHK(c, hipMemcpyAsync(n_null, c->d_grid_total, sizeof *n_null, hipMemcpyDeviceToHost, c->stream));
    return MCRAT_HIP_OK;
}
// ... then the slots themselves into null_slots[0 .. n_null); block_start: nblk + 1 + grid_scan_scratch_ints(nblk) ints, nblk = (n + 255) / 256
static int null_slots_write(mcrat_hip_ctx *c, const unsigned *block_count, unsigned long long n_null, int *block_start, int *null_slots)
{
    const long long nblk = (c->ph.n + 255) / 256;
    HIPCHK(c, launch_exclusive_scan(block_count, nblk, block_start, block_start + nblk + 1, (long long)n_null, c->stream));
    HIPCHK(c, launch_null_write(c->ph, block_start, null_slots, c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_emit_cyclosynch_pool(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, double r_inj, double ph_weight, int maximum_photons,
                                              double theta_min, double theta_max, double fps, uint64_t seed, int *num_emitted,
                                              double *ph_weight_adjusted, int *integrals_not_converged)
{
    if (!c || !cs || cs->b_field_calc < 0 || cs->b_field_calc > 2 || !(ph_weight > 0) || !(fps > 0) || maximum_photons < 0) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro || !c->hcol_buf || !c->have_photons) return MCRAT_HIP_ESTATE;
    int rc = flush_pending(c);
    if (rc) return rc;
    const int M = c->hy.M;
    const RadialRange shell = emit_shell_radii(r_inj, cs->scatt_frame_number, cs->inj_frame_number, fps);
    CsEmitParams p = cs_emit_params(c, cs);
    emit_into(p, Region{shell.rmin, shell.rmax, theta_min, theta_max, 0});
    RngKey key = c->key;
    key.seed = seed;
    const size_t need_counts = (size_t)std::max(M, (c->ph.n + 255) / 256 + 8);
    { int rc_ = ensure_counts(c, need_counts); if (rc_) return rc_; }
    DeviceTemp<unsigned> d_flags;
    HIPCHK(c, d_flags.alloc(4));
    // :1244-1296: the weight loop on the device's totals
    const double max_photons = cs->rebin_e_perc * maximum_photons;
    double weight = ph_weight;
    unsigned long long total = 0;
    unsigned flags[4] = {0, 0, 0, 0}, cells_in_shell = 0;
    bool ok = false;
    for (unsigned long long attempt = 0; attempt <= 400 && !ok; ++attempt) {
        if (hipMemsetAsync(d_flags, 0, 4 * sizeof(unsigned), c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
        if (launch_birth_count(p, c->hy, c->hcol, weight, attempt, key, c->grid_count, c->d_grid_total, d_flags, c->stream) != hipSuccess ||
            hipMemcpyAsync(&total, c->d_grid_total, sizeof total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { c->last_error = "cyclo-synchrotron emission: count pass failed"; return MCRAT_HIP_EHIP; }
        if (attempt == 0) cells_in_shell = flags[1];                                // (the kernel counts them on its first pass only)
        if (flags[0] != 0) {  // gsl_integration_qags (:1276) past its first rule AND past the device's bisection (inject.hip, qags_planck): not a result to go on with
            if (integrals_not_converged) *integrals_not_converged = (int)flags[0];
            return emit_not_converged(c, flags[0]);
        }
        const int min_photons = cells_in_shell ? 1 : 0;                             // no cell in the shell: nothing to emit (:1236-1239)
        ok = weight_search_step(total, min_photons, max_photons, &weight);
    }
    if (!ok) { c->last_error = list_refusal_text(EMIT_NO_WEIGHT); return MCRAT_HIP_EINVAL; }
    const int n_emit = (int)total;
    if (num_emitted) *num_emitted = n_emit;
    if (ph_weight_adjusted) *ph_weight_adjusted = weight;
    if (integrals_not_converged) *integrals_not_converged = (int)flags[0];
    if (n_emit == 0) return MCRAT_HIP_OK;
    // cell -> first pool photon (the counts live in grid_count[0..M)); keep them while the list may be re-allocated
    const size_t scan_ints = (size_t)M + 1 + grid_scan_scratch_ints(M);
    DeviceTemp<int> d_start;
    if (d_start.alloc(scan_ints) != hipSuccess) return MCRAT_HIP_ENOMEM;
    if (launch_exclusive_scan(c->grid_count, M, d_start, d_start + M + 1, (long long)total, c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
    // addToPhotonList (photons.c:108-208): the null slots, the list doubled first when it has none
    unsigned long long n_null = 0;
    auto count_nulls = [&]() -> int {
        if (null_slots_count(c, c->grid_count, &n_null) || hipStreamSynchronize(c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
        return MCRAT_HIP_OK;
    };
    if ((rc = count_nulls())) return rc;
    if (n_null == 0) {                                                              // num_photons >= list_capacity && num_null_photons <= num (:112)
        const long long new_cap = list_capacity_grown(c->ph.n, n_emit);
        if (new_cap > 0x7fffffffLL) return MCRAT_HIP_EINVAL;
        if ((rc = grow_photons(c, (int)new_cap))) return rc;
        if ((rc = ensure_counts(c, (size_t)((c->ph.n + 255) / 256 + 8)))) return rc;
        if ((rc = count_nulls())) return rc;
    }
    if ((unsigned long long)n_emit > n_null) { c->last_error = list_refusal_text(EMIT_NO_NULL_SLOTS); return MCRAT_HIP_EINVAL; }
    const long long nblk = (c->ph.n + 255) / 256;
    const size_t start_ints = (size_t)nblk + 1 + grid_scan_scratch_ints(nblk);
    if ((rc = ensure_aos(c, sizeof(int) * (start_ints + (size_t)n_null)))) return rc;
    int *blk_start = static_cast<int *>(c->aos_buf), *null_slots = blk_start + start_ints;
    if (null_slots_write(c, c->grid_count, n_null, blk_start, null_slots) ||
        launch_cs_emit_generate(p, c->hy, c->hcol, weight, key, d_start, n_emit, null_slots, c->ph, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { c->last_error = "cyclo-synchrotron emission: generate pass failed"; return MCRAT_HIP_EHIP; }
    c->frame_open = false;
    drop_graph(c);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_set_photons_soa(mcrat_hip_ctx *c, const mcrat_hip_photon_soa *s)
{
    if (!c || !s || s->n <= 0) return MCRAT_HIP_EINVAL;
    if (!s->type || !s->p0 || !s->p1 || !s->p2 || !s->p3 || !s->r0 || !s->r1 || !s->r2 || !s->num_scatt ||
        !s->recalc_properties || !s->weight || !s->nearest_block_index)
        return MCRAT_HIP_EINVAL;
    const int rc = alloc_photons(c, s->n);
    return rc ? rc : upload_columns(c, s);
}

extern "C" int mcrat_hip_snapshot_photons(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    if (c->parent) { c->last_error = "snapshot the pool, not one of its views"; return MCRAT_HIP_ESTATE; }
    if (int rc_ = capture_refuses(c, "snapshot_photons")) return rc_;
    if (c->frame_open && c->n_ranks == 0) { HIPCHK(c, launch_flush(c->ph, c->d_state, c->step_blocks, c->stream)); }
    if (int rc_ = ensure_device_bytes(c, &c->ph_snap, &c->ph_snap_bytes, c->ph_bytes)) return rc_;
    HIPCHK(c, hipMemcpyAsync(c->ph_snap, c->ph_buf, c->ph_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->snap_lens.clear();
    for (mcrat_hip_ctx *v : c->views) c->snap_lens.push_back((v && v->have_photons) ? v->ph.n : -1);    // lists change length (cyclo-synchrotron)
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_restore_photons(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->parent || !c->have_photons || !c->ph_snap || c->ph_snap_bytes < c->ph_bytes) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "restore_photons")) return rc_;
    HIPCHK(c, hipMemcpyAsync(c->ph_buf, c->ph_snap, c->ph_bytes, hipMemcpyDeviceToDevice, c->stream));
    c->frame_open = false;        // the loop state no longer matches the photons: begin_frame comes next
    for (size_t r = 0; r < c->views.size(); ++r) {
        mcrat_hip_ctx *v = c->views[r];
        if (!v) continue;
        v->frame_open = false;
        if (r < c->snap_lens.size() && c->snap_lens[r] >= 0) v->ph.n = c->snap_lens[r];
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_rebin_cyclosynch(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, int max_photons, int *empty_bins_out,
                                          int *num_cyclosynch_ph_emit, int *scatt_cyclosynch_num_ph)
{
    if (!c || !cs || max_photons <= 0) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    int rc = flush_pending(c);
    if (rc) return rc;
    const int n = c->ph.n, three = c->kc.dimensions == DIM_THREE;
    // collect_photon_statistics :273-322
    const int rblk = rebin_range_blocks(n);
    if ((rc = ensure_aos(c, sizeof(RebinRange) * (size_t)rblk))) return rc;
    HIPCHK(c, launch_rebin_range(c->ph, three, static_cast<RebinRange *>(c->aos_buf), c->stream));
    std::vector<RebinRange> part((size_t)rblk);
    HIPCHK(c, hipMemcpyAsync(part.data(), c->aos_buf, sizeof(RebinRange) * (size_t)rblk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const RebinRange q = rebin_range_merge(part.data(), rblk);
    // calculate_binning_params :324-347, allocate_histograms :351-391
    auto refuse = [&](ListRefusal why) { c->last_error = list_refusal_text(why); return MCRAT_HIP_EREFUSED; };
    RebinAxes ax;
    if (const ListRefusal why = rebin_axes(q, cs->rebin_e_perc, cs->rebin_ang, cs->rebin_ang_phi, max_photons, three, &ax)) return refuse(why);
    // scratch: bin of every slot, per-bin counts / cursors / starts, the member lists, the records, the null-slot list
    const int B = ax.total_bins;
    const long long nblk = (n + 255) / 256;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_bin = take(sizeof(int) * (size_t)n), o_cnt = take(sizeof(unsigned) * (size_t)(B + 2)), o_cur = take(sizeof(unsigned) * (size_t)B);
    const size_t o_start = take(sizeof(int) * ((size_t)B + 1 + grid_scan_scratch_ints(B))), o_mem = take(sizeof(int) * (size_t)n);
    const size_t o_rec = take(sizeof(RebinRec) * (size_t)B);
    const size_t o_nblk = take(sizeof(unsigned) * (size_t)(nblk + 8)), o_nstart = take(sizeof(int) * ((size_t)nblk + 1 + grid_scan_scratch_ints(nblk)));
    const size_t o_null = take(sizeof(int) * (size_t)n);
    if ((rc = ensure_aos(c, off))) return rc;
    char *b = static_cast<char *>(c->aos_buf);
    int *bin_of = reinterpret_cast<int *>(b + o_bin), *bin_start = reinterpret_cast<int *>(b + o_start), *members = reinterpret_cast<int *>(b + o_mem);
    unsigned *bin_count = reinterpret_cast<unsigned *>(b + o_cnt), *cursor = reinterpret_cast<unsigned *>(b + o_cur);
    unsigned *empty = bin_count + B;                              // [B]: empty bins, [B + 1]: photons outside the histograms
    RebinRec *recs = reinterpret_cast<RebinRec *>(b + o_rec);
    unsigned *null_cnt = reinterpret_cast<unsigned *>(b + o_nblk);
    int *null_start = reinterpret_cast<int *>(b + o_nstart), *null_slots = reinterpret_cast<int *>(b + o_null);
    if ((rc = ensure_counts(c, 1))) return rc;
    HIPCHK(c, launch_rebin_assign(c->ph, ax, bin_of, bin_count, c->stream));           // zeroes bin_count[0 .. B + 1] first
    HIPCHK(c, hipMemsetAsync(cursor, 0, sizeof(unsigned) * (size_t)B, c->stream));
    // how many photons take part (= the scan's total): eligible photons are all binned or the call fails
    std::vector<unsigned> h_cnt((size_t)B + 2);
    HIPCHK(c, hipMemcpyAsync(h_cnt.data(), bin_count, sizeof(unsigned) * ((size_t)B + 2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    long long members_total = 0;
    for (int k = 0; k < B; ++k) members_total += h_cnt[(size_t)k];
    if (h_cnt[(size_t)B + 1] != 0) return refuse(REBIN_BIN_OUT_OF_RANGE);
    HIPCHK(c, launch_exclusive_scan(bin_count, B, bin_start, bin_start + B + 1, members_total, c->stream));
    HIPCHK(c, launch_rebin_fill(c->ph, bin_of, bin_start, cursor, members, c->stream));
    HIPCHK(c, launch_rebin_create(c->ph, ax, bin_start, members, recs, empty, c->stream));
    HIPCHK(c, launch_rebin_nullify(c->ph, c->stream));                                            // :573-581
    // addToPhotonList(rebin_ph, total_bins), photons.c:108-208
    unsigned long long n_null = 0;
    unsigned h_empty[2] = {0, 0};
    if ((rc = null_slots_count(c, null_cnt, &n_null))) return rc;
    HIPCHK(c, hipMemcpyAsync(h_empty, empty, sizeof h_empty, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((unsigned long long)B > n_null) return refuse(REBIN_NO_NULL_SLOTS);
    if ((rc = null_slots_write(c, null_cnt, n_null, null_start, null_slots))) return rc;
    HIPCHK(c, launch_rebin_place(c->ph, recs, B, null_slots, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    RebinCounts after;
    if (const ListRefusal why = rebin_after(n, (long long)n_null, B, (int)h_empty[0], q.synch, &after)) return refuse(why);
    if (empty_bins_out) *empty_bins_out = after.empty_bins;
    if (scatt_cyclosynch_num_ph) *scatt_cyclosynch_num_ph = after.scatt_cyclosynch_num_ph;
    if (num_cyclosynch_ph_emit) *num_cyclosynch_ph_emit = after.num_cyclosynch_ph_emit;
    drop_graph(c);
    return MCRAT_HIP_OK;
}

// rebinCyclosynchCompPhotons (mc_cyclosynch.c:610-710) for the lists `ids` of a rank pool at once: two launches (one workgroup per list) and two
// host round trips for all of them, against a dozen launches and four round trips per list through mcrat_hip_rebin_cyclosynch on the views.
// The host's part in between -- the histograms' axes from the ranges (:324-391) -- is the same function (rebin_axes, list_plan.hpp), so a list comes
// out bit for bit the same.
// rc[j]: MCRAT_HIP_OK, or MCRAT_HIP_EREFUSED where the reference would refuse or exit (the view's last_error says why); empty / emit / scatt as
// mcrat_hip_rebin_cyclosynch returns them.  Returns the first hard error.
struct PoolRebinResult { int rc, empty_bins, num_cyclosynch_ph_emit, scatt_cyclosynch_num_ph; };
static int pool_rebin_lists(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, int max_photons, const std::vector<int> &ids, std::vector<PoolRebinResult> &res)
{
    const int L = (int)ids.size();
    res.assign((size_t)L, PoolRebinResult{MCRAT_HIP_OK, 0, 0, 0});
    if (L == 0) return MCRAT_HIP_OK;
    const int three = c->kc.dimensions == DIM_THREE;
    std::vector<RebinPoolList> h((size_t)L);
    for (int j = 0; j < L; ++j) {
        mcrat_hip_ctx *v = c->views[ids[(size_t)j]];
        int rc = flush_pending(v);
        if (rc) return rc;
        memset(&h[(size_t)j], 0, sizeof(RebinPoolList));
        h[(size_t)j].first = ids[(size_t)j] * c->rank_stride;
        h[(size_t)j].n = v->ph.n;
    }
    // launch 1: collect_photon_statistics :273-322 of every list
    const size_t o_lists = 0, o_range = align_up(sizeof(RebinPoolList) * (size_t)L, 256);
    int rc = ensure_aos(c, o_range + sizeof(RebinRange) * (size_t)L);
    if (rc) return rc;
    char *b = static_cast<char *>(c->aos_buf);
    HIPCHK(c, hipMemcpyAsync(b + o_lists, h.data(), sizeof(RebinPoolList) * (size_t)L, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rebin_pool_range(c->ph, three, reinterpret_cast<const RebinPoolList *>(b + o_lists), L, reinterpret_cast<RebinRange *>(b + o_range), c->stream));
    std::vector<RebinRange> range((size_t)L);
    HIPCHK(c, hipMemcpyAsync(range.data(), b + o_range, sizeof(RebinRange) * (size_t)L, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the host's part, list by list: calculate_binning_params :324-347, allocate_histograms :351-391
    auto refuse = [&](int j, ListRefusal why) { c->views[ids[(size_t)j]]->last_error = list_refusal_text(why); res[(size_t)j].rc = MCRAT_HIP_EREFUSED; };
    std::vector<RebinPoolList> go;
    std::vector<int> go_j;
    size_t scratch = 0;
    for (int j = 0; j < L; ++j) {
        RebinPoolList l = h[(size_t)j];
        if (const ListRefusal why = rebin_axes(range[(size_t)j], cs->rebin_e_perc, cs->rebin_ang, cs->rebin_ang_phi, max_photons, three, &l.ax)) { refuse(j, why); continue; }
        l.scratch = scratch;
        l.status = -1;
        scratch += rebin_pool_scratch_bytes(l.n, l.ax.total_bins);
        go.push_back(l);
        go_j.push_back(j);
    }
    const int G = (int)go.size();
    if (G == 0) return MCRAT_HIP_OK;
    // launch 2: everything else
    const size_t o_scr = align_up(sizeof(RebinPoolList) * (size_t)G, 256);
    if ((rc = ensure_aos(c, o_scr + scratch))) return rc;
    b = static_cast<char *>(c->aos_buf);
    HIPCHK(c, hipMemcpyAsync(b, go.data(), sizeof(RebinPoolList) * (size_t)G, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rebin_pool(c->ph, reinterpret_cast<RebinPoolList *>(b), G, b + o_scr, c->stream));
    HIPCHK(c, hipMemcpyAsync(go.data(), b, sizeof(RebinPoolList) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int g = 0; g < G; ++g) {
        const int j = go_j[(size_t)g];
        mcrat_hip_ctx *v = c->views[ids[(size_t)j]];
        const RebinPoolList &l = go[(size_t)g];
        drop_graph(v);
        if (l.status != 0 && l.status != 1 && l.status != 2) { c->last_error = "rebinning: the pool kernel left a list without a status"; return MCRAT_HIP_EHIP; }
        RebinCounts after{0, 0, 0};
        const ListRefusal why = l.status == 1 ? REBIN_BIN_OUT_OF_RANGE : l.status == 2 ? REBIN_NO_NULL_SLOTS
                                : rebin_after(l.n, l.n_null, l.ax.total_bins, l.empty_bins, range[(size_t)j].synch, &after);
        if (why) { refuse(j, why); continue; }
        res[(size_t)j].empty_bins = after.empty_bins;
        res[(size_t)j].scatt_cyclosynch_num_ph = after.scatt_cyclosynch_num_ph;
        res[(size_t)j].num_cyclosynch_ph_emit = after.num_cyclosynch_ph_emit;
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_num_photon_slots(const mcrat_hip_ctx *c) { return (c && c->have_photons) ? c->ph.n : 0; }

extern "C" int mcrat_hip_profile_totals(const mcrat_hip_ctx *c, double *loop_kernel_ms, long long *loop_kernel_launches)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->cfg.profile) return MCRAT_HIP_ESTATE;
    if (loop_kernel_ms) *loop_kernel_ms = c->prof_step_ms;
    if (loop_kernel_launches) *loop_kernel_launches = c->prof_launches;
    return MCRAT_HIP_OK;
}

static int flush_pending(mcrat_hip_ctx *c)
{
    if (c->n_ranks > 0 || (c->parent && c->rank_current)) return MCRAT_HIP_OK;      // rank_loop_kernel leaves the photons current
    if (c->pending_applied) return MCRAT_HIP_OK;  // between the two halves of a pass: the step kernel has applied it, the event kernel will replace it
    HIPCHK(c, launch_flush(c->ph, c->d_state, c->step_blocks, c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_get_photons_soa(mcrat_hip_ctx *c, const mcrat_hip_photon_soa *s)
{
    if (!c || !s) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    if (s->n != c->ph.n) return MCRAT_HIP_EINVAL;
    const int n = c->ph.n;
    int rc = flush_pending(c);
    if (rc) return rc;
    const PhotonDev &p = c->ph;
    for (int k = 0; k < N_ABI_COLS; ++k)
        if (s->*SOA_COLS[k]) HIPCHK(c, hipMemcpyAsync(s->*SOA_COLS[k], p.*PHOTON_COLS[k], sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (s->nearest_block_index) HIPCHK(c, hipMemcpyAsync(s->nearest_block_index, p.idx, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    if (s->type) HIPCHK(c, hipMemcpyAsync(s->type, p.type, n, hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned char> flags;
    if (s->recalc_properties) {
        flags.resize(n);
        HIPCHK(c, hipMemcpyAsync(flags.data(), p.flags, n, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (s->recalc_properties)
        for (int i = 0; i < n; ++i) s->recalc_properties[i] = (flags[i] & FLAG_RECALC) ? 1 : 0;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_get_photons(mcrat_hip_ctx *c, mcrat_hip_photon_list *l)
{
    if (!c || !l || !l->photons) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    if (l->list_capacity != c->ph.n) return MCRAT_HIP_EINVAL;
    const int n = c->ph.n;
    int rc = flush_pending(c);
    if (rc) return rc;
    const size_t bytes = sizeof(mcrat_hip_photon) * (size_t)n;
    const bool fresh = !c->aos_buf || c->aos_bytes < bytes || c->parent;     // (a view's staging buffer is its pool's)
    if ((rc = ensure_aos(c, bytes))) return rc;
    // photons that came in as SoA columns have no uploaded records: the bytes between the members are the caller's
    if (fresh) HIPCHK(c, hipMemcpyAsync(c->aos_buf, l->photons, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_soa_to_aos(c->ph, c->aos_buf, 0, n, c->stream));
    HIPCHK(c, hipMemcpyAsync(l->photons, c->aos_buf, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->cfg.cyclosynchrotron_switch) {          // the list changed inside the frame: the counts of photons.c:252-275
        int nulls = 0;
        for (int i = 0; i < n; ++i) nulls += l->photons[i].type == 'N';
        l->num_null_photons = nulls;
        l->num_photons = n - nulls;
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_get_photons_range(mcrat_hip_ctx *c, int first, int count, mcrat_hip_photon *records)
{
    if (!c || !records || first < 0 || count <= 0) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    if ((long long)first + count > c->ph.n) return MCRAT_HIP_EINVAL;
    int rc = flush_pending(c);
    if (rc) return rc;
    const size_t bytes = sizeof(mcrat_hip_photon) * (size_t)count;
    if ((rc = ensure_aos(c, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(c->aos_buf, 0, bytes, c->stream));        // the bytes between the members: zero
    HIPCHK(c, launch_soa_to_aos(c->ph, c->aos_buf, first, count, c->stream));
    HIPCHK(c, hipMemcpyAsync(records, c->aos_buf, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_convert_comptonized(mcrat_hip_ctx *c, int *num_converted)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    int rc = ensure_aos(c, sizeof(unsigned));
    if (rc) return rc;
    unsigned n = 0;
    HIPCHK(c, hipMemsetAsync(c->aos_buf, 0, sizeof(unsigned), c->stream));
    HIPCHK(c, launch_convert_comptonized(c->ph, static_cast<unsigned *>(c->aos_buf), c->stream));
    HIPCHK(c, hipMemcpyAsync(&n, c->aos_buf, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (num_converted) *num_converted = (int)n;
    return MCRAT_HIP_OK;
}

// the output block's scan (photon_plan.hpp, output_layout): the first output slot of each 256 slots, and the launcher's scratch
static size_t output_scan_ints(long long nblk) { return (size_t)nblk + 1 + grid_scan_scratch_ints(nblk); }
// the compacted output columns of the `total` photons with weight != 0 into the block at `base`; c->grid_count holds their number per 256 slots
static int write_output(mcrat_hip_ctx *c, const OutputLayout &lay, void *base, long long nblk, unsigned long long total, OutputCols *oc)
{
    char *b = static_cast<char *>(base);
    for (int k = 0; k < N_OUTPUT_COLS; ++k) oc->col[k] = reinterpret_cast<double *>(b + lay.col[k]);
    oc->type = b + lay.type;
    int *start = reinterpret_cast<int *>(b + lay.scan), *scratch = start + nblk + 1;
    HIPCHK(c, launch_exclusive_scan(c->grid_count, nblk, start, scratch, (long long)total, c->stream));
    HIPCHK(c, launch_output_write(c->ph, c->ph.n, start, *oc, c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_get_output(mcrat_hip_ctx *c, mcrat_hip_output_columns *out)
{
    if (!c || !out) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    const int n = c->ph.n;
    int rc = flush_pending(c);
    if (rc) return rc;
    const long long nblk = (n + 255) / 256;
    { int rc_ = ensure_counts(c, (size_t)nblk); if (rc_) return rc_; }
    unsigned long long total = 0;
    HIPCHK(c, launch_output_count(c->ph, n, c->grid_count, c->d_grid_total, c->stream));
    HIPCHK(c, hipMemcpyAsync(&total, c->d_grid_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int m = (int)total;
    bool any = out->type != nullptr;
    for (int k = 0; k < N_OUTPUT_COLS; ++k) any = any || out->*OUTPUT_COLS[k];
    if (!any) { out->count = m; return MCRAT_HIP_OK; }            // sizing call
    if (out->count < m) { out->count = m; return MCRAT_HIP_EINVAL; }
    out->count = m;
    if (m == 0) return MCRAT_HIP_OK;
    const OutputLayout lay = output_layout((size_t)m, output_scan_ints(nblk), 0);
    if ((rc = ensure_aos(c, lay.total))) return rc;
    OutputCols oc;
    if ((rc = write_output(c, lay, c->aos_buf, nblk, total, &oc))) return rc;
    for (int k = 0; k < N_OUTPUT_COLS; ++k)
        if (out->*OUTPUT_COLS[k]) HIPCHK(c, hipMemcpyAsync(out->*OUTPUT_COLS[k], oc.col[k], sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (out->type) HIPCHK(c, hipMemcpyAsync(out->type, oc.type, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- asynchronous output
// What saveCheckpoint (mcrat_io.c:838-1009) and printPhotons (mcrat_io.c:114-836) read, taken off the device WHILE THE NEXT FRAME RUNS: post()
// stages the records and the compacted output columns in device buffers of the outbox by kernels in the context's stream order -- the photons
// may change as soon as post() has returned -- and a copy stream of the outbox's own brings them into pinned host memory; wait() (any thread)
// blocks until they have landed.  (The reference writes both files at the end of every frame with its rank idle, mcrat.c:902,907.)
struct mcrat_hip_outbox {
    int device = 0;
    hipStream_t copy = nullptr;
    hipEvent_t staged = nullptr, landed = nullptr;
    void *d_buf = nullptr, *h_buf = nullptr;
    size_t d_bytes = 0, h_bytes = 0;
    OutputLayout lay{};               // of the last post, in both buffers
    int n_records = 0, n_output = 0;
    bool posted = false, have_records = false, have_output = false;
};

extern "C" int mcrat_hip_outbox_create(mcrat_hip_ctx *c, mcrat_hip_outbox **out)
{
    if (!c || !out) return MCRAT_HIP_EINVAL;
    mcrat_hip_outbox *b = new (std::nothrow) mcrat_hip_outbox();
    if (!b) return MCRAT_HIP_ENOMEM;
    b->device = c->cfg.device;
    if (hipStreamCreateWithFlags(&b->copy, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&b->staged, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b->landed, hipEventDisableTiming) != hipSuccess) {
        mcrat_hip_outbox_destroy(b);
        return MCRAT_HIP_EHIP;
    }
    *out = b;
    return MCRAT_HIP_OK;
}

extern "C" void mcrat_hip_outbox_destroy(mcrat_hip_outbox *b)
{
    if (!b) return;
    if (b->copy) { (void)hipStreamSynchronize(b->copy); (void)hipStreamDestroy(b->copy); }
    if (b->staged) (void)hipEventDestroy(b->staged);
    if (b->landed) (void)hipEventDestroy(b->landed);
    if (b->d_buf) (void)hipFree(b->d_buf);
    if (b->h_buf) (void)hipHostFree(b->h_buf);
    delete b;
}

extern "C" int mcrat_hip_outbox_post(mcrat_hip_ctx *c, mcrat_hip_outbox *b, int want_records, int want_output)
{
    if (!c || !b || (!want_records && !want_output)) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    const int n = c->ph.n;
    int rc = flush_pending(c);
    if (rc) return rc;
    if (b->posted) HIPCHK(c, hipEventSynchronize(b->landed));          // (a post over one nobody waited for)
    b->posted = false;
    const long long nblk = (n + 255) / 256;
    unsigned long long total = 0;
    if (want_output) {
        int rc_ = ensure_counts(c, (size_t)nblk);
        if (rc_) return rc_;
        HIPCHK(c, launch_output_count(c->ph, n, c->grid_count, c->d_grid_total, c->stream));
        HIPCHK(c, hipMemcpyAsync(&total, c->d_grid_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const size_t m = (size_t)total;
    const OutputLayout lay = output_layout(m, output_scan_ints(nblk), want_records ? n : 0, want_output != 0);
    const size_t room = lay.total > b->d_bytes ? lay.total + lay.total / 4 : lay.total;        // (grown with a quarter to spare)
    if ((rc = ensure_device_bytes(c, &b->d_buf, &b->d_bytes, room)) || (rc = ensure_host_bytes(c, &b->h_buf, &b->h_bytes, room))) return rc;
    char *d = static_cast<char *>(b->d_buf);
    b->lay = lay;
    b->n_records = want_records ? n : 0;
    b->n_output = (int)m;
    b->have_records = want_records != 0;
    b->have_output = want_output != 0;
    if (want_records) {
        HIPCHK(c, hipMemsetAsync(d + lay.rec, 0, lay.rec_bytes, c->stream));                   // the bytes between the members: zero
        HIPCHK(c, launch_soa_to_aos(c->ph, d + lay.rec, 0, n, c->stream));
    }
    OutputCols oc;
    if (want_output && m > 0 && (rc = write_output(c, lay, d, nblk, total, &oc))) return rc;
    HIPCHK(c, hipEventRecord(b->staged, c->stream));
    HIPCHK(c, hipStreamWaitEvent(b->copy, b->staged, 0));
    if (lay.copy_bytes) HIPCHK(c, hipMemcpyAsync(b->h_buf, d, lay.copy_bytes, hipMemcpyDeviceToHost, b->copy));
    HIPCHK(c, hipEventRecord(b->landed, b->copy));
    b->posted = true;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_outbox_wait(mcrat_hip_outbox *b, const mcrat_hip_photon **records, int *n_records, mcrat_hip_output_columns *cols)
{
    if (!b) return MCRAT_HIP_EINVAL;
    if (!b->posted) return MCRAT_HIP_ESTATE;
    if (hipSetDevice(b->device) != hipSuccess) return MCRAT_HIP_ENODEV;       // (the caller may be a thread of its own)
    if (hipEventSynchronize(b->landed) != hipSuccess) return MCRAT_HIP_EHIP;
    char *h = static_cast<char *>(b->h_buf);
    if (records) *records = b->have_records ? reinterpret_cast<const mcrat_hip_photon *>(h + b->lay.rec) : nullptr;
    if (n_records) *n_records = b->n_records;
    if (cols) {
        memset(cols, 0, sizeof *cols);
        cols->count = b->have_output ? b->n_output : 0;
        if (b->have_output && b->n_output > 0) bind_output(b->lay, h, cols);
    }
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- the loop
static long long read_table_fallbacks(mcrat_hip_ctx *c)
{
    int m = 0;
    if (c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && c->d_table_fallbacks &&
        hipMemcpy(&m, c->d_table_fallbacks, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) m = -1;
    return m;
}

static void fill_stats(mcrat_hip_ctx *c, mcrat_hip_frame_stats *s)
{
    if (!s) return;
    const LoopState &h = *c->h_state;
    s->iterations = h.iterations;
    s->photon_steps = h.iterations * (long long)c->ph.n;
    s->slot_steps = h.slot_steps;
    s->frame_scatt_cnt = h.frame_scatt_cnt;
    s->num_photons_find_new_element = h.n_relocated;
    s->not_found = h.not_found;
    s->kn_rejections = h.kn_rejections;
    s->rescans = h.rescans;
    s->last_scattered_index = h.last_scattered_index;
    s->last_scattered_temp = h.last_scattered_temp;
    s->last_time_step = h.last_time_step;
    s->remaining_time = h.remaining_time;
    s->time_now = h.time_now;
    s->step_kernel_ms = c->prof_step_ms;
    s->step_kernel_launches = c->prof_launches;
    s->event_kernel_ms = c->prof_event_ms;
    s->table_fallbacks = read_table_fallbacks(c);
}

static void state_to_stats(const LoopState &h, long long slots, mcrat_hip_frame_stats *s)
{
    memset(s, 0, sizeof *s);
    s->iterations = h.iterations;
    s->photon_steps = h.iterations * slots;
    s->slot_steps = h.slot_steps;
    s->frame_scatt_cnt = h.frame_scatt_cnt;
    s->num_photons_find_new_element = h.n_relocated;
    s->not_found = h.not_found;
    s->kn_rejections = h.kn_rejections;
    s->rescans = h.rescans;
    s->last_scattered_index = h.last_scattered_index;
    s->last_scattered_temp = h.last_scattered_temp;
    s->last_time_step = h.last_time_step;
    s->remaining_time = h.remaining_time;
    s->time_now = h.time_now;
}

// the same from a frame queue's record (frame_queue.hpp, FrameRecord)
static void record_to_stats(const FrameRecord &h, long long slots, mcrat_hip_frame_stats *s)
{
    memset(s, 0, sizeof *s);
    s->iterations = h.iterations;
    s->photon_steps = h.iterations * slots;
    s->slot_steps = h.slot_steps;
    s->frame_scatt_cnt = h.frame_scatt_cnt;
    s->num_photons_find_new_element = h.n_relocated;
    s->not_found = h.not_found;
    s->kn_rejections = h.kn_rejections;
    s->rescans = h.rescans;
    s->last_scattered_index = h.last_scattered_index;
    s->last_scattered_temp = h.last_scattered_temp;
    s->last_time_step = h.last_time_step;
    s->remaining_time = h.remaining_time;
    s->time_now = h.time_now;
}

// ... and the host's copy of a list's LoopState as the frame that left the record left it: everything the host reads of it (state_to_stats, done); the
// members only the kernel uses stay on the device (states[rank]), the state of a finished frame holds no pending advance
static void record_to_state(const FrameRecord &h, LoopState *s)
{
    memset(s, 0, sizeof *s);
    s->remaining_time = h.remaining_time; s->time_now = h.time_now; s->done = h.done; s->skip_idx = -1; s->last_scattered_index = h.last_scattered_index;
    s->last_time_step = h.last_time_step; s->last_scattered_temp = h.last_scattered_temp; s->iterations = h.iterations; s->frame_scatt_cnt = h.frame_scatt_cnt;
    s->n_relocated = h.n_relocated; s->not_found = h.not_found; s->kn_rejections = h.kn_rejections; s->rescans = h.rescans; s->slot_steps = h.slot_steps;
}

static int rank_slots(const mcrat_hip_ctx *c, int r)
{
    if (c->is_pool) return c->h_desc[r].len;
    const int per = c->cfg.virtual_rank_photons;
    return std::min(per, c->ph.n - r * per);
}

static int longest_rank_list(const mcrat_hip_ctx *c)
{
    if (!c->is_pool) return std::min(c->cfg.virtual_rank_photons, c->ph.n);
    int m = 0;
    for (int r = 0; r < c->n_ranks; ++r) m = std::max(m, c->h_desc[r].len);
    return m;
}

// whole-job view of the virtual ranks: counters add up; the clock shown is that of the rank furthest behind
static void fill_rank_stats(mcrat_hip_ctx *c, mcrat_hip_frame_stats *s)
{
    if (!s) return;
    mcrat_hip_frame_stats t, acc;
    memset(&acc, 0, sizeof acc);
    for (int r = 0; r < c->n_ranks; ++r) {
        state_to_stats(c->h_rstates[r], rank_slots(c, r), &t);
        acc.iterations += t.iterations; acc.photon_steps += t.photon_steps; acc.slot_steps += t.slot_steps; acc.frame_scatt_cnt += t.frame_scatt_cnt;
        acc.num_photons_find_new_element += t.num_photons_find_new_element; acc.not_found += t.not_found;
        acc.kn_rejections += t.kn_rejections; acc.rescans += t.rescans;
        if (r == 0 || t.remaining_time > acc.remaining_time) {
            acc.remaining_time = t.remaining_time; acc.time_now = t.time_now; acc.last_time_step = t.last_time_step;
            acc.last_scattered_index = t.last_scattered_index; acc.last_scattered_temp = t.last_scattered_temp;
        }
    }
    *s = acc;
}

#ifdef MCRAT_DIAG
extern "C" __attribute__((visibility("default"))) int mcrat_hip_diag_rank_stamps(mcrat_hip_ctx *c, int rank, long long out[8])
{
    if (!c || !out || rank < 0 || rank >= c->n_ranks) return -1;
    LoopState h;
    if (hipMemcpy(&h, c->d_rstates + rank, sizeof(LoopState), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int k = 0; k < 8; ++k) out[k] = h.stamps[k];
    return 0;
}

extern "C" __attribute__((visibility("default"))) int mcrat_hip_diag_stamps(mcrat_hip_ctx *c, long long out[8])
{
    if (!c || !out) return -1;
    if (hipMemcpy(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int k = 0; k < 8; ++k) out[k] = c->h_state->stamps[k];
    return 0;
}
#endif

extern "C" int mcrat_hip_num_virtual_ranks(const mcrat_hip_ctx *c) { return c ? c->n_ranks : 0; }

extern "C" int mcrat_hip_rank_stats(mcrat_hip_ctx *c, int rank, mcrat_hip_frame_stats *stats)
{
    if (!c || !stats) return MCRAT_HIP_EINVAL;
    if (c->n_ranks <= 0 || !c->frame_open) return MCRAT_HIP_ESTATE;
    if (rank < 0 || rank >= c->n_ranks) return MCRAT_HIP_EINVAL;
    HIPCHK(c, hipMemcpyAsync(c->h_rstates, c->d_rstates, sizeof(LoopState) * c->n_ranks, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    state_to_stats(c->h_rstates[rank], rank_slots(c, rank), stats);
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- rank pool
static void drop_pool_tapes(mcrat_hip_ctx *c)
{
    if (c->d_pool_tape) { (void)hipFree(c->d_pool_tape); c->d_pool_tape = nullptr; }
    if (c->d_pool_tapes) { (void)hipFree(c->d_pool_tapes); c->d_pool_tapes = nullptr; }
}

extern "C" int mcrat_hip_pool_create(mcrat_hip_ctx *c, int n_ranks, int slots_per_rank)
{
    if (!c || n_ranks <= 0 || slots_per_rank <= 0) return MCRAT_HIP_EINVAL;
    if (c->parent) { c->last_error = "a rank view cannot hold a pool"; return MCRAT_HIP_ESTATE; }
    if (c->sc_world > 0) { c->last_error = "shared clock and rank pool exclude each other"; return MCRAT_HIP_ESTATE; }
    if (c->d_tape) { c->last_error = "a context with a tape of uniforms holds one list (mcrat_hip_set_rng_tape)"; return MCRAT_HIP_ESTATE; }
    const size_t stride = align_up((size_t)slots_per_rank, 2 * STEP_BLOCK);
    if (stride * (size_t)n_ranks > 0x7fffffffull - 2 * STEP_BLOCK) { c->last_error = "rank pool: more than 2^31 slots"; return MCRAT_HIP_EINVAL; }
    for (mcrat_hip_ctx *v : c->views)
        if (v) { v->parent = nullptr; destroy_view(v); }
    c->views.clear();
    c->is_pool = false;
    drop_pool_tapes(c);                              // (they were the old lists')
    c->cfg.virtual_rank_photons = (int)stride;
    int rc = alloc_photons(c, (int)(stride * (size_t)n_ranks));       // zeroed: no slot belongs to a list yet
    if (rc) return rc;
    c->is_pool = true;
    c->views.assign((size_t)n_ranks, nullptr);
    if (c->d_desc) { HIPCHK(c, hipFree(c->d_desc)); c->d_desc = nullptr; }
    if (c->h_desc) { HIPCHK(c, hipHostFree(c->h_desc)); c->h_desc = nullptr; }
    HIPCHK(c, hipMalloc((void **)&c->d_desc, sizeof(RankDesc) * (size_t)n_ranks));
    HIPCHK(c, hipHostMalloc((void **)&c->h_desc, sizeof(RankDesc) * (size_t)n_ranks, hipHostMallocDefault));
    memset(c->h_desc, 0, sizeof(RankDesc) * (size_t)n_ranks);
    HIPCHK(c, hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)n_ranks, hipMemcpyHostToDevice, c->stream));
    memset(c->h_rstates, 0, sizeof(LoopState) * (size_t)n_ranks);
    for (int r = 0; r < n_ranks; ++r) { c->h_rstates[r].done = 1; c->h_rstates[r].skip_idx = -1; c->h_rstates[r].last_scattered_index = -1; }
    HIPCHK(c, hipMemcpyAsync(c->d_rstates, c->h_rstates, sizeof(LoopState) * (size_t)n_ranks, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    photons_are_set(c);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_pool_rank(mcrat_hip_ctx *c, int rank, uint32_t rng_stream, mcrat_hip_ctx **view)
{
    if (!c || !view) return MCRAT_HIP_EINVAL;
    *view = nullptr;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (rank < 0 || rank >= c->n_ranks) return MCRAT_HIP_EINVAL;
    mcrat_hip_ctx *v = c->views[rank];
    if (!v) {
        v = new (std::nothrow) mcrat_hip_ctx();
        if (!v) return MCRAT_HIP_ENOMEM;
        v->cfg = c->cfg;
        v->cfg.virtual_rank_photons = 0;
        v->cfg.stream = c->stream;
        v->kc = c->kc;
        v->stream = c->stream;
        v->own_stream = false;
        v->parent = c;
        v->view_rank = rank;
        v->d_state = c->d_rstates + rank;         // windows into the pool's blocks; nothing here is owned by the view
        v->h_state = c->h_rstates + rank;
        v->d_red = c->d_red; v->h_red = c->h_red;
        v->d_table_fallbacks = c->d_table_fallbacks;
        c->views[rank] = v;
        sync_views(c);
    }
    v->cfg.rng_stream = rng_stream;
    v->key.stream = rng_stream & 0xffffffu;
    v->view_stream = v->key.stream;
    *view = v;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_pool_layout(const mcrat_hip_ctx *c, int *n_ranks, int *slots_per_rank)
{
    if (!c || !c->is_pool) return MCRAT_HIP_ESTATE;
    if (n_ranks) *n_ranks = c->n_ranks;
    if (slots_per_rank) *slots_per_rank = c->rank_stride;
    return MCRAT_HIP_OK;
}

// mcrat_hip_begin_frame for many views in one launch: every list with open[r] != 0 gets its own seed and clock
extern "C" int mcrat_hip_pool_begin_frames(mcrat_hip_ctx *c, const int *open, const uint64_t *seeds, const double *time_now, const double *remaining_time)
{
    if (!c || !open || !seeds || !time_now || !remaining_time) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "pool_begin_frames")) return rc_;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    if (c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && !c->d_hot_table) {
        c->last_error = "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first";
        return MCRAT_HIP_ESTATE;
    }
    const int R = c->n_ranks;
    std::vector<int> op((size_t)R, 0);
    for (int r = 0; r < R; ++r) {
        mcrat_hip_ctx *v = c->views[r];
        if (!open[r]) continue;
        if (!v || !v->have_photons) { c->last_error = "pool_begin_frames: a list that does not exist was asked to open a frame"; return MCRAT_HIP_ESTATE; }
        op[(size_t)r] = 1;
    }
    const size_t bytes = (sizeof(int) + 2 * sizeof(double)) * (size_t)R;
    int rc = ensure_aos(c, bytes + 64);
    if (rc) return rc;
    double *d_t = static_cast<double *>(c->aos_buf), *d_rem = d_t + R;
    int *d_open = reinterpret_cast<int *>(d_rem + R);
    HIPCHK(c, hipMemcpyAsync(d_t, time_now, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rem, remaining_time, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_open, op.data(), sizeof(int) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_table_fallbacks, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_init_states_multi(c->d_rstates, R, d_open, d_t, d_rem, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));        // the arrays above are the caller's and `op`
    for (int r = 0; r < R; ++r) {
        if (!op[(size_t)r]) continue;
        mcrat_hip_ctx *v = c->views[r];
        if (v->graph_exec && v->key.seed != seeds[r]) drop_graph(v);
        v->key.seed = seeds[r];
        v->find_switch = 1;
        v->pending_applied = false;
        v->rank_current = false;
        v->frame_open = true;
        v->prof_step_ms = v->prof_event_ms = 0;
        v->prof_launches = 0;
        LoopState &h = *v->h_state;
        memset(&h, 0, sizeof h);
        h.remaining_time = remaining_time[r]; h.time_now = time_now[r]; h.done = !(remaining_time[r] > 0);
        h.skip_idx = -1; h.last_scattered_index = -1; h.force_relocate = 1;
    }
    c->rank_block_fixed = false;
    return MCRAT_HIP_OK;
}

// the loop statistics of every list (what mcrat_hip_frame_statistics gives for one view), one read-back
extern "C" int mcrat_hip_pool_frame_stats(mcrat_hip_ctx *c, mcrat_hip_frame_stats *out)
{
    if (!c || !out) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    HIPCHK(c, hipMemcpyAsync(c->h_rstates, c->d_rstates, sizeof(LoopState) * (size_t)c->n_ranks, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->n_ranks; ++r) {
        const mcrat_hip_ctx *v = c->views[r];
        state_to_stats(c->h_rstates[r], (v && v->have_photons) ? v->ph.n : 0, &out[r]);
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_pool_summaries(mcrat_hip_ctx *c, mcrat_hip_rank_summary *out)
{
    if (!c || !out) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    const int R = c->n_ranks;
    for (int r = 0; r < R; ++r) {                  // every list that exists, whether or not it is in a frame
        const mcrat_hip_ctx *v = c->views[r];
        RankDesc d{};
        if (v && v->have_photons) { d.len = v->ph.n; d.stream = v->key.stream; d.seed = v->key.seed; }
        c->h_desc[r] = d;
    }
    const size_t bytes = (sizeof(ReducePartial) + sizeof(int)) * (size_t)R + sizeof(RankDesc) * (size_t)R;
    int rc = ensure_aos(c, bytes);
    if (rc) return rc;
    ReducePartial *d_part = static_cast<ReducePartial *>(c->aos_buf);
    RankDesc *d_desc = reinterpret_cast<RankDesc *>(d_part + R);
    int *d_nout = reinterpret_cast<int *>(d_desc + R);
    HIPCHK(c, hipMemcpyAsync(d_desc, c->h_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_rank_reduce(c->ph, c->rank_stride, R, d_desc, d_part, d_nout, c->cfg.cyclosynchrotron_switch, c->stream));
    std::vector<ReducePartial> part((size_t)R);
    std::vector<int> nout((size_t)R);
    HIPCHK(c, hipMemcpyAsync(part.data(), d_part, sizeof(ReducePartial) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nout.data(), d_nout, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < R; ++r) {
        const ReducePartial &t = part[(size_t)r];
        mcrat_hip_rank_summary &o = out[r];
        memset(&o, 0, sizeof o);
        o.list_capacity = c->h_desc[r].len;
        if (o.list_capacity <= 0) continue;
        o.min_r = t.r_min; o.max_r = t.r_max; o.min_theta = t.th_min; o.max_theta = t.th_max;
        o.max_scatt = (int)t.max_scatt; o.min_scatt = (int)t.min_scatt;
        o.avg_scatt = t.sum_scatt / (double)t.count; o.avg_r = t.sum_r / (double)t.count;
        o.avg_energy = (t.e_sum * C_LIGHT) / t.w_sum;
        o.num_output = nout[(size_t)r];
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_begin_frame(mcrat_hip_ctx *c, uint64_t seed, double time_now, double remaining_time)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro || !c->have_photons) return MCRAT_HIP_ESTATE;
    if (c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && !c->d_hot_table) {
        c->last_error = "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first";
        return MCRAT_HIP_ESTATE;
    }
    // everything below is ordered on the context's stream behind whatever the previous frame left there: no wait
    HIPCHK(c, hipMemsetAsync(c->d_table_fallbacks, 0, sizeof(int), c->stream));
    LoopState h;
    memset(&h, 0, sizeof h);
    h.remaining_time = remaining_time;
    h.time_now = time_now;
    h.done = !(remaining_time > 0);
    h.skip_idx = -1;
    h.last_scattered_index = -1;
    if (c->parent) h.force_relocate = 1;           // a view's LoopState is the pool's for this list (rank_loop_kernel looks at the flag)
    HIPCHK(c, launch_init_states(c->d_state, c->d_rstates, c->n_ranks, h, c->stream));     // per list: force_relocate = 1, mcrat.c:756
    if (c->is_pool)                                // the pool's own begin_frame: every list, the same seed and clock
        for (mcrat_hip_ctx *v : c->views)
            if (v && v->have_photons) { v->key.seed = seed; v->frame_open = true; v->find_switch = 1; v->pending_applied = false; v->rank_current = false; }
    *c->h_state = h;                               // the host's view until the next read-back (every read-back is followed by a wait)
    HIPCHK(c, hipMemsetAsync(c->shortlist, 0, sizeof(Shortlist), c->stream));
    if (c->sc_world > 0) HIPCHK(c, hipMemsetAsync(c->d_sc, 0, sizeof(ScState), c->stream));
    if (c->graph_exec && c->key.seed != seed) drop_graph(c);      // the captured launches carry the key by value
    c->key.seed = seed;
    c->find_switch = 1;           // mcrat.c:756
    c->pending_applied = false;
    c->rank_current = false;
    c->rank_block_fixed = false;
    c->frame_open = true;
    c->prof_step_ms = c->prof_event_ms = 0;
    c->prof_launches = 0;
    return MCRAT_HIP_OK;
}

// the event half of a pass from the context's random source: the keyed streams, or the caller's tape (then preceded by the pass's free-path
// draws in slot order, kernels.hip tape_draw_kernel)
static hipError_t launch_event_of(mcrat_hip_ctx *c)
{
    if (c->d_tape) {
        TapeDev t;
        t.u = c->d_tape; t.n = c->tape_n; t.cursor = c->d_tape_cursor; t.error = reinterpret_cast<int *>(c->d_tape_cursor + 1);
        return launch_tape_pass(c->kc, c->ph, c->hy, c->d_state, c->key, t, c->partials, c->step_blocks, c->shortlist, c->stream);
    }
    return launch_event(c->kc, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream);
}

static int launch_iteration(mcrat_hip_ctx *c, bool force)
{
    HIPCHK(c, launch_step(c->kc, force, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream));
    HIPCHK(c, launch_event_of(c));
    return MCRAT_HIP_OK;
}

// The random stream as an INPUT (SURVEY.md section 8c "tape").  MCRaT draws everything from one sequential ranlxs0 stream
// (mcrat.c:99-103,701); a maintainer who records that stream (tools/ref_harness: the doubles the generator returned, in call order) hands it
// over here and the loop consumes it exactly as MCRaT does -- one gsl_rng_uniform_pos per located slot in ascending slot order
// (mclib.c:646-675), then photonEvent's draws (electron.c:81,196,217-233; mcrat_scattering.c:519-574), gsl_rng_uniform_pos skipping zeros and the
// polar Gaussian taking as many pairs as it needs -- so that photons can be compared with MCRaT's own, photon for photon.  A validation mode: one
// list per context (no rank pool, no shared clock, no cyclo-synchrotron hook), the free-path draws of a pass walked by one workgroup.
// n == 0 (or uniforms == NULL) returns the context to its keyed streams.  The seed of begin_frame is ignored while a tape is set.
extern "C" int mcrat_hip_set_rng_tape(mcrat_hip_ctx *c, const double *uniforms, long long n)
{
    if (!c || n < 0) return MCRAT_HIP_EINVAL;
    if (c->parent || c->is_pool || c->n_ranks > 0 || c->cfg.virtual_rank_photons > 0 || c->sc_world > 0 || c->cfg.cyclosynchrotron_switch) {
        c->last_error = "the tape of uniforms is for one list with one clock (no rank pool, virtual ranks, shared clock or cyclo-synchrotron hook)";
        return MCRAT_HIP_ESTATE;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drop_graph(c);
    if (c->d_tape) { (void)hipFree(c->d_tape); c->d_tape = nullptr; c->tape_n = 0; }
    if (!uniforms || n == 0) return MCRAT_HIP_OK;
    for (long long k = 0; k < n; ++k)
        if (!(uniforms[k] >= 0.0 && uniforms[k] < 1.0)) { c->last_error = "the tape holds a value outside [0, 1)"; return MCRAT_HIP_EINVAL; }
    if (!c->d_tape_cursor) HIPCHK(c, hipMalloc((void **)&c->d_tape_cursor, 2 * sizeof(long long)));
    HIPCHK(c, hipMemset(c->d_tape_cursor, 0, 2 * sizeof(long long)));
    HIPCHK(c, hipMalloc((void **)&c->d_tape, sizeof(double) * (size_t)n));
    HIPCHK(c, hipMemcpy(c->d_tape, uniforms, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    c->tape_n = n;
    return MCRAT_HIP_OK;
}

// how far the tape has been read (entries consumed so far, zeros skipped by uniform_pos included); *ran_out != 0: the loop needed more entries
// than the tape holds (its results are then meaningless).  Synchronises the stream.
extern "C" int mcrat_hip_rng_tape_position(mcrat_hip_ctx *c, long long *position, int *ran_out)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->d_tape) return MCRAT_HIP_ESTATE;
    long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->d_tape_cursor, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (position) *position = h[0];
    if (ran_out) *ran_out = (int)(h[1] & 0xffffffffll) != 0;
    return MCRAT_HIP_OK;
}

// The tape for the lists of a rank pool: per list, the doubles MCRaT's generator returned for that rank (tools/ref_harness; every MPI rank has its own
// stream, mcrat.c:99-103,701), consumed as mcrat_hip_set_rng_tape consumes one -- by the tape build of the loop kernel (kernels.hip,
// rank_loop_kernel<.., TAPE>), which every frame of a pool that holds tapes runs through.  uniforms[k] == NULL or n[k] == 0: list k keeps its keyed
// streams.  Replaces every list's tape; positions start at 0.  A taped list ignores its seed.
extern "C" int mcrat_hip_pool_set_rng_tapes(mcrat_hip_ctx *c, const double *const *uniforms, const long long *n)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->parent || !c->is_pool) { c->last_error = "tapes for many lists are set on a rank pool (mcrat_hip_set_rng_tape: one list)"; return MCRAT_HIP_ESTATE; }
    if (c->cfg.cyclosynchrotron_switch) { c->last_error = "CYCLOSYNCHROTRON_SWITCH is on: the cyclo-synchrotron hook has no tape build"; return MCRAT_HIP_ESTATE; }
    if (!uniforms || !n) return MCRAT_HIP_EINVAL;
    const int R = c->n_ranks;
    long long total = 0;
    for (int r = 0; r < R; ++r) {
        if (n[r] < 0) return MCRAT_HIP_EINVAL;
        if (!uniforms[r]) continue;
        for (long long k = 0; k < n[r]; ++k)
            if (!(uniforms[r][k] >= 0.0 && uniforms[r][k] < 1.0)) { c->last_error = "a tape holds a value outside [0, 1)"; return MCRAT_HIP_EINVAL; }
        total += n[r];
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drop_pool_tapes(c);
    if (total == 0) return MCRAT_HIP_OK;
    std::vector<TapeList> h((size_t)R);
    memset(h.data(), 0, sizeof(TapeList) * (size_t)R);
    double *buf = nullptr;
    HIPCHK(c, hipMalloc((void **)&buf, sizeof(double) * (size_t)total));
    c->d_pool_tape = buf;
    long long off = 0;
    for (int r = 0; r < R; ++r) {
        if (!uniforms[r] || n[r] == 0) continue;
        h[(size_t)r].offset = off;
        h[(size_t)r].n = n[r];
        HIPCHK(c, hipMemcpy(buf + off, uniforms[r], sizeof(double) * (size_t)n[r], hipMemcpyHostToDevice));
        off += n[r];
    }
    TapeList *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, sizeof(TapeList) * (size_t)R));
    c->d_pool_tapes = d;
    HIPCHK(c, hipMemcpy(d, h.data(), sizeof(TapeList) * (size_t)R, hipMemcpyHostToDevice));
    return MCRAT_HIP_OK;
}

// per list: entries of its tape read so far (zeros skipped by uniform_pos included; 0 for a keyed list) and whether it needed more than its tape
// holds (its results are then meaningless).  Synchronises the stream.
extern "C" int mcrat_hip_pool_rng_tape_positions(mcrat_hip_ctx *c, long long *position, int *ran_out)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->parent || !c->is_pool || !c->d_pool_tapes) { c->last_error = "no rank pool with tapes (mcrat_hip_pool_set_rng_tapes)"; return MCRAT_HIP_ESTATE; }
    const int R = c->n_ranks;
    std::vector<TapeList> h((size_t)R);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_pool_tapes, sizeof(TapeList) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < R; ++r) {
        if (position) position[r] = h[(size_t)r].cursor;
        if (ran_out) ran_out[r] = h[(size_t)r].error != 0;
    }
    return MCRAT_HIP_OK;
}

static int ensure_events(mcrat_hip_ctx *c, size_t n)
{
    while (c->ev.size() < n) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->ev.push_back(e);
    }
    return MCRAT_HIP_OK;
}

static int ensure_graph(mcrat_hip_ctx *c, int batch)
{
    if (c->graph_exec && c->graph_batch == batch) return MCRAT_HIP_OK;
    drop_graph(c);
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = MCRAT_HIP_OK;
    for (int b = 0; b < batch && rc == MCRAT_HIP_OK; ++b) rc = launch_iteration(c, false);
    hipError_t e = hipStreamEndCapture(c->stream, &c->graph);
    if (rc != MCRAT_HIP_OK) return rc;
    HIPCHK(c, e);
    HIPCHK(c, hipGraphInstantiate(&c->graph_exec, c->graph, nullptr, nullptr, 0));
    c->graph_batch = batch;
    return MCRAT_HIP_OK;
}

static int ensure_events(mcrat_hip_ctx *c, size_t n);

// cfg.profile: the duration of `launches` launches, between two events, added to prof_step_ms.  `launch` queues them; `wait`, if given, queues what
// goes behind them and waits for the stream (so that the read-back is in flight before the host waits); either returns an MCRAT_HIP_ code.
template <class Launch, class Wait>
static int profiled(mcrat_hip_ctx *c, int launches, Launch &&launch, Wait &&wait)
{
    const bool on = c->cfg.profile != 0;
    int rc = on ? ensure_events(c, 2) : MCRAT_HIP_OK;
    if (rc) return rc;
    if (on) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    if ((rc = launch())) return rc;
    if (on) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    if ((rc = wait())) return rc;
    if (on) {
        float ms = 0;
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        c->prof_step_ms += ms;
        c->prof_launches += launches;
    }
    return MCRAT_HIP_OK;
}
template <class Launch>
static int profiled(mcrat_hip_ctx *c, int launches, Launch &&launch) { return profiled(c, launches, launch, [] { return MCRAT_HIP_OK; }); }

// virtual-rank mode: every launch gives each unfinished list up to `per_launch` passes of its own loop
// the device as the context has known it since its creation (a view asks its pool's)
static const RankDeviceInfo *device_info(const mcrat_hip_ctx *c)
{
    if (c->dev.cus <= 0 && c->parent) c = c->parent;
    return c->dev.cus > 0 ? &c->dev : nullptr;
}
static int device_cus(const mcrat_hip_ctx *c)
{
    if (const RankDeviceInfo *d = device_info(c)) return d->cus;
    int cus = 256, dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}

// MCRAT_HIP_RANK_BLOCK and MCRAT_HIP_RANK_FUSE as the block rules read them
static RankEnv rank_env()
{
    RankEnv env;
    if (const char *e = getenv("MCRAT_HIP_RANK_BLOCK")) { env.block_set = true; env.block = atoi(e); }
    if (const char *e = getenv("MCRAT_HIP_RANK_FUSE")) { env.fuse_set = true; env.fuse = atoi(e); }
    return env;
}
// threads per list and the fused pass for the next launches (rank_form_plan.hpp, rank_block_rule)
static void choose_rank_block(mcrat_hip_ctx *c)
{
    const RankBlock b = rank_block_rule(c->n_ranks, device_cus(c), longest_rank_list(c), c->rank_passes_per_list, c->kc.geometry, rank_env());
    c->rank_block = b.threads; c->rank_fuse = b.fuse;
}

// passes one list may take per launch: bounds one launch to a second or two even for the densest lists (4096: the first 60 frames of
// tools/lundman_run.py, 9.3e6 scatterings in the first one, 9.3 -> 8.9 s)
static long long rank_launch_cap()
{
    const char *e = getenv("MCRAT_HIP_RANK_LAUNCH_CAP");
    return e && atoll(e) > 0 ? atoll(e) : 32768;
}

// a launch of the context's lists in the form chosen for them (choose_rank_block, or the cyclo-synchrotron pool's own choice)
static RankLaunch rank_launch_of(const mcrat_hip_ctx *c, const RankDesc *desc, long long max_passes)
{
    RankLaunch rl;
    rl.n_ranks = c->n_ranks; rl.rank_stride = c->rank_stride; rl.longest_list = longest_rank_list(c); rl.desc = desc;
    rl.threads = c->rank_block; rl.fuse = c->rank_fuse;
    rl.no_lds_lists = getenv("MCRAT_HIP_NO_LDS_LISTS") != nullptr;    // (read per launch: tests flip it between the launches of one process)
    rl.max_passes = max_passes;
    rl.dev = device_info(c);
    return rl;
}

// rank pool: what the kernel needs to know about every list, from its view
static int pool_describe(mcrat_hip_ctx *c)
{
    for (int r = 0; r < c->n_ranks; ++r) {
        const mcrat_hip_ctx *v = r < (int)c->views.size() ? c->views[r] : nullptr;
        RankDesc d{};
        if (v && v->have_photons && v->frame_open) { d.len = v->ph.n; d.stream = v->key.stream; d.seed = v->key.seed; }
        c->h_desc[r] = d;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)c->n_ranks, hipMemcpyHostToDevice, c->stream));
    return MCRAT_HIP_OK;
}

// Launch `rl` (its max_passes: the most one launch gives a list) through hydro frame `hy` until every open list is done -- of a pool: every window
// with a list in it, h_desc[r].len > 0 --, or, with max_iterations > 0, until the lists have been given that many passes.  A pool that holds tapes runs
// the tape build, whatever the form.  *all_done: every open list is done; h_rstates holds the lists' states either way.
static int run_lists(mcrat_hip_ctx *c, const HydroDev &hy, RankLaunch rl, long long max_iterations, bool *all_done)
{
    const long long cap = rl.max_passes;
    *all_done = false;
    for (long long it = 0; !*all_done && (max_iterations <= 0 || it < max_iterations); it += rl.max_passes) {
        rl.max_passes = (max_iterations > 0 && cap > max_iterations - it) ? max_iterations - it : cap;
        int rc = profiled(c, 1, [&]() -> int {
            if (c->d_pool_tapes)
                HIPCHK(c, launch_rank_loop_tape(c->kc, c->ph, hy, c->d_rstates, c->key, c->n_ranks, c->rank_stride, c->d_desc, c->d_pool_tape, c->d_pool_tapes,
                                                rl.max_passes, c->stream));
            else
                HIPCHK(c, launch_rank_loop(c->kc, c->ph, hy, c->d_rstates, c->key, rl, c->stream));
            return MCRAT_HIP_OK;
        }, [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(c->h_rstates, c->d_rstates, sizeof(LoopState) * (size_t)c->n_ranks, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return MCRAT_HIP_OK;
        });
        if (rc) return rc;
        *all_done = true;
        for (int r = 0; r < c->n_ranks && *all_done; ++r) {
            if (c->is_pool && c->h_desc[r].len <= 0) continue;     // a window without a list (or without a frame) has nothing to finish
            *all_done = c->h_rstates[r].done != 0;
        }
    }
    return MCRAT_HIP_OK;
}

static int run_ranks(mcrat_hip_ctx *c, long long max_iterations, mcrat_hip_frame_stats *stats)
{
    if (c->is_pool) { int rc = pool_describe(c); if (rc) return rc; }
    if (!c->rank_block_fixed) { choose_rank_block(c); c->rank_block_fixed = true; }    // one choice per frame (begin_frame resets)
    bool all_done = false;
    int rc = run_lists(c, c->hy, rank_launch_of(c, c->is_pool ? c->d_desc : nullptr, rank_launch_cap()), max_iterations, &all_done);
    if (rc) return rc;
    if (all_done && c->is_pool)
        for (mcrat_hip_ctx *v : c->views)
            if (v && v->frame_open) v->rank_current = true;
    fill_rank_stats(c, stats);
    {   // what the next frame's choice of workgroup size looks at
        long long it_sum = 0;
        bool done = true;
        for (int r = 0; r < c->n_ranks; ++r) { it_sum += c->h_rstates[r].iterations; done = done && c->h_rstates[r].done; }
        if (done && c->n_ranks > 0) c->rank_passes_per_list = (double)it_sum / c->n_ranks;
    }
    if (stats) { stats->step_kernel_ms = c->prof_step_ms; stats->step_kernel_launches = c->prof_launches; stats->table_fallbacks = read_table_fallbacks(c); }
    return MCRAT_HIP_OK;
}

// ------------------------------------------------------------------ the frame queue's host side (mcrat_hip_pool_run_frames)
// The call's scratch lives on the context (fq_*): no allocation per call once a plan of this size has been seen.

// MCRAT_HIP_QUEUE_TIMING=1: where the call's host time goes, on stderr (development aid)
struct QueueMarks {
    double start, checked = 0, items = 0, chosen = 0, ordered = 0, launched = 0, synced = 0;      // us
    size_t bytes_up = 0, bytes_down = 0;
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    QueueMarks() : start(now()) {}
};

// The plan's arguments and the state it needs; the staged hydro frames of the plan into fq_hyv: index 0 the pool's own, then every other context named
// in plan->hydro (it keeps its frame staged while the call runs; same switches as the pool -- its HydroDev is handed to the pool's kernels as it is)
static int frames_check(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, const mcrat_hip_frame_stats *stats)
{
    if (!c || !p || !stats || p->n_frames <= 0 || !p->open || !p->seeds || !p->time_now || !p->remaining_time) return MCRAT_HIP_EINVAL;
    if (p->chain_clock && !p->frame_end) return MCRAT_HIP_EINVAL;
    if (int rc_ = capture_refuses(c, "pool_run_frames")) return rc_;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    if (c->cfg.cyclosynchrotron_switch) { c->last_error = "CYCLOSYNCHROTRON_SWITCH is on: its hook needs the host between passes, one frame per call (mcrat_hip_pool_scatter_frames_cyclosynch)"; return MCRAT_HIP_ESTATE; }
    if (c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && !c->d_hot_table) {
        c->last_error = "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first";
        return MCRAT_HIP_ESTATE;
    }
    std::vector<HydroDev> &hyv = c->fq_hyv;
    std::vector<const mcrat_hip_ctx *> &hy_ctx = c->fq_hy_ctx;
    hyv.assign(1, c->hy);
    hy_ctx.assign(1, c);
    c->fq_hy_of_frame.assign((size_t)p->n_frames, 0);
    if (p->hydro)
        for (int f = 0; f < p->n_frames; ++f) {
            const mcrat_hip_ctx *o = p->hydro[f];
            if (!o || o == c) continue;
            if (!o->have_hydro) { c->last_error = "pool_run_frames: a context named in plan->hydro holds no staged frame"; return MCRAT_HIP_ESTATE; }
            if (o->kc.dimensions != c->kc.dimensions || o->kc.geometry != c->kc.geometry || o->kc.table != c->kc.table || o->cfg.device != c->cfg.device) {
                c->last_error = "pool_run_frames: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY, TAU_CALCULATION) or on another device";
                return MCRAT_HIP_EINVAL;
            }
            if (c->kc.table && !o->hy.hot_table) { c->last_error = "pool_run_frames: TAU_CALCULATION == TABLE and a frame's context has no cross-section table"; return MCRAT_HIP_ESTATE; }
            size_t k = 1;
            while (k < hy_ctx.size() && hy_ctx[k] != o) ++k;
            if (k == hy_ctx.size()) { hy_ctx.push_back(o); hyv.push_back(o->hy); }
            c->fq_hy_of_frame[(size_t)f] = (int)k;
        }
    if ((size_t)c->n_ranks * (size_t)p->n_frames > 0x7fffffffull) return MCRAT_HIP_EINVAL;
    return MCRAT_HIP_OK;
}

static int frames_ensure_block(mcrat_hip_ctx *c, size_t bytes)
{
    if (c->fq_bytes >= bytes) return MCRAT_HIP_OK;
    if (c->d_fq) { HIPCHK(c, hipFree(c->d_fq)); c->d_fq = nullptr; }
    if (c->h_fq) { HIPCHK(c, hipHostFree(c->h_fq)); c->h_fq = nullptr; }
    c->fq_bytes = 0;
    HIPCHK(c, hipMalloc(&c->d_fq, bytes));
    HIPCHK(c, hipHostMalloc(&c->h_fq, bytes, hipHostMallocDefault));
    c->fq_bytes = bytes;
    return MCRAT_HIP_OK;
}

// One pass over the plan into the pinned block: the items (every member written: nothing of the block is cleared but the ticket and frames_done words),
// the lists that take part, each in one run of consecutive frames (fq_first, fq_last), their descriptions, and the hydro frames.
static int frames_fill(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, const FrameQueueLayout &lay)
{
    const int R = c->n_ranks, F = p->n_frames;
    FrameItem *items = lay.items(c->h_fq);
    std::vector<int> &first = c->fq_first, &last = c->fq_last;
    first.assign((size_t)R, -1);
    last.assign((size_t)R, -1);
    for (int f = 0; f < F; ++f) {
        const size_t t0 = (size_t)f * R;
        const int hydro_f = c->fq_hy_of_frame[(size_t)f];
        for (int r = 0; r < R; ++r) {
            const size_t t = t0 + r;
            FrameItem &it = items[t];
            it.seed = p->seeds[t]; it.time_now = p->time_now[t]; it.remaining_time = p->remaining_time[t];
            it.frame_end = p->frame_end ? p->frame_end[t] : 0.0;
            it.open = p->open[t] ? 1 : 0;
            it.hydro = hydro_f;
            if (!it.open) continue;
            if (first[r] < 0) first[r] = f;
            else if (last[r] != f - 1) { c->last_error = "pool_run_frames: a list's open frames must be consecutive"; return MCRAT_HIP_EINVAL; }
            last[r] = f;
        }
    }
    for (int r = 0; r < R; ++r) {
        const mcrat_hip_ctx *v = c->views[(size_t)r];
        if (first[r] >= 0 && (!v || !v->have_photons)) { c->last_error = "pool_run_frames: a list that does not exist was asked to open a frame"; return MCRAT_HIP_ESTATE; }
    }
    if (p->restore_each_frame) {
        if (!c->ph_snap || c->ph_snap_bytes < c->ph_bytes) { c->last_error = "pool_run_frames: restore_each_frame without a snapshot (mcrat_hip_snapshot_photons)"; return MCRAT_HIP_ESTATE; }
        for (int r = 0; r < R; ++r)
            if (first[r] >= 0 && ((size_t)r >= c->snap_lens.size() || c->snap_lens[(size_t)r] != c->views[(size_t)r]->ph.n)) {
                c->last_error = "pool_run_frames: a list has changed length since the snapshot";
                return MCRAT_HIP_ESTATE;
            }
    }
    RankDesc *qdesc = lay.desc(c->h_fq);
    for (int r = 0; r < R; ++r) {                            // (the queue's kernel reads the block's copy; the context's host copy is what the launch form is chosen from)
        const mcrat_hip_ctx *v = c->views[(size_t)r];
        RankDesc d{};
        if (first[r] >= 0) { d.len = v->ph.n; d.stream = v->key.stream; d.seed = p->seeds[(size_t)first[r] * R + r]; }
        c->h_desc[r] = d;
        qdesc[r] = d;
    }
    memcpy(lay.hydro(c->h_fq), c->fq_hyv.data(), sizeof(HydroDev) * c->fq_hyv.size());
    memset(static_cast<char *>(c->h_fq) + lay.words.off, 0, lay.words.bytes);
    return MCRAT_HIP_OK;
}

// The queue as the kernel gets it (all but the order's offsets), and the captures' buffer: with plan->capture_frames, the lists as every frame but the
// last leaves them (the frame's outputs: mcrat.c:881-915)
static int frames_queue_dev(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, const FrameQueueLayout &lay, bool host_records, FrameQueueDev *fq)
{
    const int F = p->n_frames;
    *fq = FrameQueueDev{};
    fq->n_frames = F; fq->restore = p->restore_each_frame ? 1 : 0; fq->chain_clock = p->chain_clock ? 1 : 0;
    fq->ticket = lay.ticket(c->d_fq); fq->frames_done = lay.frames_done(c->d_fq);
    fq->order = lay.order(c->d_fq); fq->items = lay.items(c->d_fq); fq->hydro = lay.hydro(c->d_fq);
    fq->records = lay.records(c->d_fq);
    if (host_records) {                                      // (the pinned block as the device sees it)
        void *mapped = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&mapped, c->h_fq, 0));
        fq->records = lay.records(mapped);
    }
    fq->snap_delta = p->restore_each_frame ? image_delta(c->ph_snap, c->ph_buf, 0, c->ph_bytes) : 0;
    c->cap_frames = 0;
    if (p->capture_frames && F > 1) {
        if (int rc = ensure_device_bytes(c, &c->ph_cap, &c->ph_cap_bytes, c->ph_bytes * (size_t)(F - 1))) return rc;
        fq->capture_delta = image_delta(c->ph_cap, c->ph_buf, 0, c->ph_bytes);
        fq->capture_stride = (long long)c->ph_bytes;          // (image_delta's block_bytes: the kernel adds frame * capture_stride itself)
        c->cap_frames = F - 1;
        // a capture holds the slots [0, list_capacity) of the lists that were open in its frame; every other slot must read as the empty slot it is in
        // the live lists (printPhotons' compaction keeps weight != 0 over the whole pool): the weight column starts from zero
        for (int f = 0; f < F - 1; ++f)
            HIPCHK(c, hipMemsetAsync(shift_photons(c->ph, image_delta(c->ph_cap, c->ph_buf, f, c->ph_bytes)).weight, 0, sizeof(double) * (size_t)c->ph.n, c->stream));
    }
    return MCRAT_HIP_OK;
}

// Queue launches until every list is through its last frame: order the open items, one copy up, the launch, one copy down, and what the launch left
// (frame_queue.hpp).  The caller has asked the rule that the launch form has a queue build; *unsupported (hipErrorNotSupported from the first launch)
// is left for the runtime refusing that build its LDS: nothing has run then.
static int frames_run_queue(mcrat_hip_ctx *c, const FrameQueueLayout &lay, FrameQueueDev &fq, RankLaunch rl, bool host_records, QueueMarks &tm, bool *unsupported)
{
    const int R = c->n_ranks, F = fq.n_frames;
    char *hb = static_cast<char *>(c->h_fq), *db = static_cast<char *>(c->d_fq);
    int xcd_of_class[FRAME_QUEUE_XCDS];
    for (int x = 0; x < FRAME_QUEUE_XCDS; ++x) xcd_of_class[x] = x;
    c->fq_stalled.assign((size_t)R, -1);
    rl.desc = lay.desc(c->d_fq);
    rl.fq = &fq;
    // (the records the kernel stored into the pinned block itself: tickets and frames_done alone come back)
    const FrameQueueLayout::Range down = host_records ? lay.words : lay.down;
    *unsupported = false;
    constexpr int NO_QUEUE_BUILD = 1;                        // (beside the MCRAT_HIP_ codes, which are <= 0: nothing was launched)
    for (int attempt = 0;; ++attempt) {
        rl.n_open = frame_queue_groups(frame_queue_order(lay.items(hb), R, F, xcd_of_class, lay.order(hb), fq.order_off));
        if (rl.n_open == 0) break;                           // (no list opens a frame: the call has only sized the queue's buffers)
        tm.ordered = QueueMarks::now();
        HIPCHK(c, hipMemcpyAsync(db + lay.up.off, hb + lay.up.off, lay.up.bytes, hipMemcpyHostToDevice, c->stream));
        tm.bytes_up += lay.up.bytes;
        int rc = profiled(c, 1, [&]() -> int {
            const hipError_t le = launch_rank_loop(c->kc, c->ph, c->hy, c->d_rstates, c->key, rl, c->stream);
            if (le == hipErrorNotSupported && attempt == 0) return NO_QUEUE_BUILD;
            HIPCHK(c, le);
            return MCRAT_HIP_OK;
        }, [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(hb + down.off, db + down.off, down.bytes, hipMemcpyDeviceToHost, c->stream));
            tm.bytes_down += down.bytes;
            tm.launched = QueueMarks::now();
            HIPCHK(c, hipStreamSynchronize(c->stream));
            tm.synced = QueueMarks::now();
            return MCRAT_HIP_OK;
        });
        if (rc == NO_QUEUE_BUILD) { *unsupported = true; return MCRAT_HIP_OK; }
        if (rc) return rc;
        const FrameQueueNext next = frame_queue_after_launch(lay.frames_done(hb), lay.ticket(hb), lay.records(hb), lay.items(hb), R, c->fq_first.data(),
                                                             c->fq_last.data(), fq.chain_clock != 0, c->fq_stalled.data(), xcd_of_class);
        if (next == FRAME_QUEUE_DONE) break;
        if (next == FRAME_QUEUE_NO_DRAW) { c->last_error = "pool_run_frames: no workgroup drew an item"; return MCRAT_HIP_EHIP; }
        if (attempt >= 1 << 16) { c->last_error = "pool_run_frames: lists that make no progress"; return MCRAT_HIP_EHIP; }
    }
    return MCRAT_HIP_OK;
}

// The plan one launch per frame: launch forms without a queue build (128- and 512-thread lists, lists whose columns stay in HBM/L2, the tape build) --
// the same frames, seeds and clocks, so the same photons; what is lost is only that a list need not wait for the others at a frame's end.
static int frames_run_one_by_one(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, const FrameQueueLayout &lay, RankLaunch rl)
{
    const int R = c->n_ranks, F = p->n_frames;
    const FrameItem *items = lay.items(c->h_fq);
    FrameRecord *rec = lay.records(c->h_fq);
    const std::vector<int> &first = c->fq_first;
    std::vector<double> t_now((size_t)R, 0.0), t_rem((size_t)R, 0.0);
    std::vector<int> op((size_t)R, 0);
    const size_t sb = (sizeof(int) + 2 * sizeof(double)) * (size_t)R;
    int rc = ensure_aos(c, sb + 64);
    if (rc) return rc;
    double *d_t = static_cast<double *>(c->aos_buf), *d_rem = d_t + R;
    int *d_open = reinterpret_cast<int *>(d_rem + R);
    const char *snap = static_cast<const char *>(c->ph_snap);
    char *live = static_cast<char *>(c->ph_buf);
    rl.desc = c->d_desc;
    for (int f = 0; f < F; ++f) {
        bool any = false, all_lists = true;                               // (every list that exists takes part: the whole pool is restored in one copy)
        for (int r = 0; r < R; ++r)
            if (c->views[(size_t)r] && c->views[(size_t)r]->have_photons && !items[(size_t)f * R + r].open) all_lists = false;
        if (p->restore_each_frame && all_lists) HIPCHK(c, hipMemcpyAsync(c->ph_buf, c->ph_snap, c->ph_bytes, hipMemcpyDeviceToDevice, c->stream));
        for (int r = 0; r < R; ++r) {
            const size_t t = (size_t)f * R + r;
            op[(size_t)r] = items[t].open ? 1 : 0;
            if (!op[(size_t)r]) { c->h_desc[r].len = 0; continue; }
            any = true;
            const mcrat_hip_ctx *v = c->views[(size_t)r];
            c->h_desc[r].len = v->ph.n; c->h_desc[r].stream = v->key.stream; c->h_desc[r].seed = items[t].seed;
            t_now[(size_t)r] = items[t].time_now; t_rem[(size_t)r] = items[t].remaining_time;
            if (p->chain_clock && f > first[r]) { t_now[(size_t)r] = rec[t - R].time_now; t_rem[(size_t)r] = items[t].frame_end - t_now[(size_t)r]; }
            if (p->restore_each_frame && !all_lists) {                    // the list's window of every column back from the snapshot
                CopyExtent ext[N_WINDOW_EXTENTS];
                window_extents(c->ph_lay, (size_t)r * (size_t)c->rank_stride, (size_t)v->ph.n, ext);
                for (const CopyExtent &e : ext)
                    if (e.rows > 1) HIPCHK(c, hipMemcpy2DAsync(live + e.off, e.pitch, snap + e.off, e.pitch, e.width, e.rows, hipMemcpyDeviceToDevice, c->stream));
                    else HIPCHK(c, hipMemcpyAsync(live + e.off, snap + e.off, e.width, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        if (!any) continue;
        HIPCHK(c, hipMemcpyAsync(d_t, t_now.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_rem, t_rem.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_open, op.data(), sizeof(int) * (size_t)R, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_init_states_multi(c->d_rstates, R, d_open, d_t, d_rem, c->stream));
        bool all_done = false;                                            // (a pool that holds tapes: each frame reads on from each list's position)
        if ((rc = run_lists(c, c->fq_hyv[(size_t)c->fq_hy_of_frame[(size_t)f]], rl, 0, &all_done))) return rc;
        for (int r = 0; r < R; ++r)
            if (op[(size_t)r]) rec[(size_t)f * R + r].from_state(c->h_rstates[r]);
        if (c->cap_frames > 0 && f < F - 1)               // the pool as frame f leaves it
            HIPCHK(c, hipMemcpyAsync(live + image_delta(c->ph_cap, live, f, c->ph_bytes), live, c->ph_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    // the lists' descriptions as a queue launch leaves them: every list of the plan with its length, also one that sat the last frame out
    // (mcrat_hip_rank_stats prices a list's passes with it)
    const RankDesc *qdesc = lay.desc(c->h_fq);
    for (int r = 0; r < R; ++r) c->h_desc[r] = qdesc[r];
    return MCRAT_HIP_OK;
}

// The records as the call's statistics, and the pool as after the last frame's mcrat_hip_run
static void frames_publish(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, const FrameRecord *rec, mcrat_hip_frame_stats *stats)
{
    const int R = c->n_ranks;
    const size_t N = (size_t)R * (size_t)p->n_frames;
    for (size_t t = 0; t < N; ++t) {
        const int r = (int)(t % (size_t)R);
        if (p->open[t]) record_to_stats(rec[t], c->views[(size_t)r]->ph.n, &stats[t]);
        else memset(&stats[t], 0, sizeof stats[t]);
    }
    long long it_sum = 0;
    int lists = 0;
    for (int r = 0; r < R; ++r) {
        if (c->fq_first[(size_t)r] < 0) continue;
        mcrat_hip_ctx *v = c->views[(size_t)r];
        const size_t t = (size_t)c->fq_last[(size_t)r] * R + r;
        if (v->graph_exec && v->key.seed != p->seeds[t]) drop_graph(v);
        v->key.seed = p->seeds[t];
        v->find_switch = 1;
        v->pending_applied = false;
        v->rank_current = true;
        v->frame_open = true;
        v->prof_step_ms = v->prof_event_ms = 0;
        v->prof_launches = 0;
        record_to_state(rec[t], &c->h_rstates[r]);            // (the host's copy of the list's state: what the statistics and `done` are read from)
        it_sum += rec[t].iterations;
        lists += 1;
    }
    if (lists > 0) { c->rank_passes_per_list = (double)it_sum / lists; c->frame_open = true; }
    c->rank_block_fixed = false;
    stats[0].step_kernel_ms = c->prof_step_ms;               // (profile = 1: the launch's duration, on the first item)
    stats[0].step_kernel_launches = c->prof_launches;
    if (c->kc.table) {                                       // (the call's off-table look-ups, over every staged frame's counter)
        const std::vector<HydroDev> &hyv = c->fq_hyv;
        long long fallbacks = 0;
        for (size_t k = 0; k < hyv.size(); ++k) {
            const HydroDev &h = hyv[k];
            bool seen = false;                               // (a pool that shares another context's frame counts on that context's counter)
            for (size_t j = 0; j < k; ++j) seen = seen || hyv[j].table_fallbacks == h.table_fallbacks;
            int m = 0;
            if (!h.table_fallbacks || seen) continue;
            if (hipMemcpy(&m, h.table_fallbacks, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { fallbacks = -1; break; }
            fallbacks += m;
        }
        stats[0].table_fallbacks = fallbacks;
    }
}

// The frame queue (frame_queue.hpp; kernels.hip, rank_loop_kernel): the pool's lists through several hydro frames in one launch.
extern "C" int mcrat_hip_pool_run_frames(mcrat_hip_ctx *c, const mcrat_hip_frame_plan *p, mcrat_hip_frame_stats *stats)
{
    static const bool timing = env_flag("MCRAT_HIP_QUEUE_TIMING");
    // MCRAT_HIP_QUEUE_HOST_RECORDS=1 (A/B): the kernel stores the records straight into the pinned host block instead of device memory + one copy back
    static const bool host_records = env_flag("MCRAT_HIP_QUEUE_HOST_RECORDS");
    QueueMarks tm;
    int rc = frames_check(c, p, stats);
    if (rc) return rc;
    const int R = c->n_ranks, F = p->n_frames;
    const FrameQueueLayout lay(R, F, c->fq_hyv.size());
    if ((rc = frames_ensure_block(c, lay.bytes))) return rc;
    tm.checked = QueueMarks::now();
    if ((rc = frames_fill(c, p, lay))) return rc;
    tm.items = QueueMarks::now();
    // TAU_CALCULATION == TABLE: a frame's off-table look-ups count on the context its hydro frame is staged on (HydroDev::table_fallbacks); every
    // such counter starts the call from zero and the call reports their sum (DIRECT: no kernel touches the counters and nobody reads them)
    if (c->kc.table) {
        HIPCHK(c, hipMemsetAsync(c->d_table_fallbacks, 0, sizeof(int), c->stream));
        for (const HydroDev &h : c->fq_hyv)
            if (h.table_fallbacks) HIPCHK(c, hipMemsetAsync(h.table_fallbacks, 0, sizeof(int), c->stream));
    }
    if (!c->rank_block_fixed) { choose_rank_block(c); c->rank_block_fixed = true; }
    tm.chosen = QueueMarks::now();
    FrameQueueDev fq;
    if ((rc = frames_queue_dev(c, p, lay, host_records, &fq))) return rc;
    // passes one list may take per frame and launch (run_ranks' bound on a launch's duration)
    const RankLaunch rl = rank_launch_of(c, nullptr, rank_launch_cap());
    c->prof_step_ms = 0; c->prof_launches = 0;
    // (MCRAT_HIP_NO_FRAME_QUEUE=1, A/B: the plan frame by frame; a pool that holds tapes: the tape build has no queue form; nor have the 128- and
    // 512-thread lists and those whose columns stay in HBM/L2: rank_form_plan.hpp)
    bool one_by_one = env_flag("MCRAT_HIP_NO_FRAME_QUEUE") || c->d_pool_tapes != nullptr || rank_form_resolve(rank_form_request(c->kc, rl, true)).no_queue_build;
    if (!one_by_one && (rc = frames_run_queue(c, lay, fq, rl, host_records, tm, &one_by_one))) return rc;
    if (one_by_one && (rc = frames_run_one_by_one(c, p, lay, rl))) return rc;
    frames_publish(c, p, lay.records(c->h_fq), stats);
    if (timing)
        fprintf(stderr, "pool_run_frames: %d frames x %d lists: plan -> queue %.0f us (checks %.0f, items %.0f, memsets + block choice %.0f, order %.0f), upload + launch calls %.0f us, waiting for the device %.0f us (kernel %.0f us), records -> stats %.0f us; %zu B up, %zu B down in %lld launch(es)%s\n",
                F, R, tm.ordered - tm.start, tm.checked - tm.start, tm.items - tm.checked, tm.chosen - tm.items, tm.ordered - tm.chosen, tm.launched - tm.ordered,
                tm.synced - tm.launched, 1e3 * c->prof_step_ms, QueueMarks::now() - tm.synced, tm.bytes_up, tm.bytes_down, c->prof_launches,
                host_records ? ", records stored into the pinned block" : "");
    return MCRAT_HIP_OK;
}

// The pool's read entry points (mcrat_hip_pool_summaries, mcrat_hip_outbox_post, mcrat_hip_get_photons_range, mcrat_hip_get_output) on the lists as
// frame `frame` of the last plan left them: the captures are laid out like the live lists, so the pool's column pointers are simply moved over.
extern "C" int mcrat_hip_pool_select_frame(mcrat_hip_ctx *c, int frame)
{
    if (!c || !c->is_pool) return MCRAT_HIP_EINVAL;
    if (c->selected_frame >= 0) { c->ph = c->ph_live; c->selected_frame = -1; }
    if (frame < 0) return MCRAT_HIP_OK;
    if (frame >= c->cap_frames || !c->ph_cap) { c->last_error = "pool_select_frame: no capture of that frame (mcrat_hip_frame_plan.capture_frames; the last frame is the live lists)"; return MCRAT_HIP_ESTATE; }
    c->ph_live = c->ph;
    c->ph = shift_photons(c->ph_live, image_delta(c->ph_cap, c->ph_buf, frame, c->ph_bytes));
    c->selected_frame = frame;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_run(mcrat_hip_ctx *c, long long max_iterations, mcrat_hip_frame_stats *stats)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (int rc_ = capture_refuses(c, "run")) return rc_;
    if (c->is_pool) {                              // every list whose view has opened a frame (or the pool's own begin_frame: all)
        if (!c->have_hydro) return MCRAT_HIP_ESTATE;
        if (c->cfg.cyclosynchrotron_switch) { c->last_error = "CYCLOSYNCHROTRON_SWITCH is on: run the views one by one (mcrat_hip_scatter_frame_cyclosynch)"; return MCRAT_HIP_ESTATE; }
        c->frame_open = true;
        return run_ranks(c, max_iterations, stats);
    }
    if (!c->frame_open) return MCRAT_HIP_ESTATE;
    if (c->sc_world > 0) { c->last_error = "shared clock attached: drive the frame with mcrat_hip_shared_clock_*"; return MCRAT_HIP_ESTATE; }
    if (c->cfg.cyclosynchrotron_switch) {
        c->last_error = "CYCLOSYNCHROTRON_SWITCH is on: drive the frame with mcrat_hip_scatter_frame_cyclosynch (the loop has the hook of mcrat.c:786-808)";
        return MCRAT_HIP_ESTATE;
    }
    if (c->n_ranks > 0) return run_ranks(c, max_iterations, stats);
    if (c->parent && c->parent->d_pool_tapes) {
        c->last_error = "the pool holds tapes of uniforms (mcrat_hip_pool_set_rng_tapes): run the pool, whose tape build reads them, not one of its views";
        return MCRAT_HIP_ESTATE;
    }
    const int per_sync = c->cfg.iterations_per_sync;
    long long it = 0;
    int rc;
    while (max_iterations <= 0 || it < max_iterations) {
        int batch = per_sync;
        if (max_iterations > 0 && (long long)batch > max_iterations - it) batch = (int)(max_iterations - it);
        if (c->cfg.profile) {
            if ((rc = ensure_events(c, (size_t)3 * batch))) return rc;
            for (int b = 0; b < batch; ++b) {
                HIPCHK(c, hipEventRecord(c->ev[3 * b], c->stream));
                HIPCHK(c, launch_step(c->kc, c->find_switch != 0, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream));
                c->find_switch = 0;
                HIPCHK(c, hipEventRecord(c->ev[3 * b + 1], c->stream));
                HIPCHK(c, launch_event_of(c));
                HIPCHK(c, hipEventRecord(c->ev[3 * b + 2], c->stream));
            }
        } else {
            int b = 0;
            if (c->find_switch) {             // the forced-relocation pass is never part of the graph
                if ((rc = launch_iteration(c, true))) return rc;
                c->find_switch = 0;
                b = 1;
            }
            if (c->cfg.use_graph && b == 0 && batch == per_sync) {
                if ((rc = ensure_graph(c, batch))) return rc;
                HIPCHK(c, hipGraphLaunch(c->graph_exec, c->stream));
            } else {
                for (; b < batch; ++b)
                    if ((rc = launch_iteration(c, false))) return rc;
            }
        }
        it += batch;
        HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->cfg.profile) {
            // only launches that did work are counted: after `done` the kernels return at once
            const long long did = c->h_state->iterations - c->prof_launches;
            for (int b = 0; b < batch && b < did; ++b) {
                float ms = 0;
                HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3 * b], c->ev[3 * b + 1]));
                c->prof_step_ms += ms;
                HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3 * b + 1], c->ev[3 * b + 2]));
                c->prof_event_ms += ms;
            }
            c->prof_launches = c->h_state->iterations;
        }
        if (c->h_state->done) break;
    }
    if ((rc = flush_pending(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fill_stats(c, stats);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_propagate_frame(mcrat_hip_ctx *c, double *time_now, double remaining_time, uint64_t seed,
                                         mcrat_hip_frame_stats *stats)
{
    if (!c || !time_now) return MCRAT_HIP_EINVAL;
    int rc = mcrat_hip_begin_frame(c, seed, *time_now, remaining_time);
    if (rc) return rc;
    mcrat_hip_frame_stats local;
    rc = mcrat_hip_run(c, 0, &local);
    if (rc) return rc;
    *time_now = local.time_now;
    if (stats) *stats = local;
    return MCRAT_HIP_OK;
}

static int fast_refusals(mcrat_hip_ctx *c)
{
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    if (c->cfg.cyclosynchrotron_switch) { c->last_error = "FAST mode has no cyclo-synchrotron hooks: use the exact scatter frame"; return MCRAT_HIP_ESTATE; }
    if (c->sc_world > 0) { c->last_error = "shared clock attached: drive the frame with mcrat_hip_shared_clock_*"; return MCRAT_HIP_ESTATE; }
    if (c->cfg.tau_calculation == MCRAT_HIP_TAU_TABLE && !c->d_hot_table) {
        c->last_error = "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first";
        return MCRAT_HIP_ESTATE;
    }
    return MCRAT_HIP_OK;
}

static void fast_stats(const FastCounts &fc, double time_now, mcrat_hip_frame_stats *stats)
{
    memset(stats, 0, sizeof *stats);
    stats->iterations = (long long)fc.passes;
    stats->photon_steps = (long long)fc.photon_steps;
    stats->slot_steps = (long long)fc.photon_steps;
    stats->frame_scatt_cnt = (long long)fc.scatterings;
    stats->kn_rejections = (long long)fc.kn_rejections;
    stats->num_photons_find_new_element = (long long)fc.relocated;
    stats->not_found = (long long)fc.not_found;
    stats->last_scattered_index = -1;
    stats->remaining_time = 0;
    stats->time_now = time_now;
}

// FAST mode's refresh cadence when the caller does not name one (fast_windows <= 0).  The exact loop re-locates a photon and redraws its free
// path whenever ANY photon of its rank scatters -- N_events(rank, frame) times per frame, for the reference's ranks of about 1000 photons that
// is the frame's scatterings per 1000 photons.  A fixed 8 is right for thin frames and biased by a per cent in dense ones (the Lundman run's first
// frames: 68.0 scatterings per photon against the exact mode's 67.3; 128 windows give 67.3).  So the cadence follows the frame: the scatterings per
// 1000 photons the LIST's last fast frame counted (fast_cadence_learn below), between 8 and 2048, 32 before any frame has run.
static int fast_cadence(const mcrat_hip_ctx *c, int fast_windows)
{
    return fast_windows > 0 ? fast_windows : c->fast_auto_windows;
}
// The cadence is a property of the LIST (kept on its context -- a pool's list: on its view): what a 10^3-photon rank of the exact mode would have
// refreshed in the frame this list has just seen -- its own scatterings per thousand of its own photons, between 8 and 2048 windows.  A list's
// photons therefore do not depend on which other lists share its pool, and mcrat_hip_fast_cadence carries the value over a restart.
static void fast_cadence_learn(mcrat_hip_ctx *c, unsigned long long scatterings, long long photons)
{
    if (photons <= 0) return;
    const double per_thousand = 1000.0 * (double)scatterings / (double)photons;
    // (the upper end: at 7 300 scatterings per thousand photons and frame 128 windows still count 0.14 % too many scatterings, 512 0.05 %, 2048 none --
    // tools/fast_cadence_gate.py, 1.9e7 events -- and 2048 windows are still faster than the exact loop there)
    c->fast_auto_windows = per_thousand < 8.0 ? 8 : (per_thousand > 2048.0 ? 2048 : (int)(per_thousand + 0.5));
}

extern "C" int mcrat_hip_fast_cadence(mcrat_hip_ctx *c, int set_windows)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (set_windows > 0) c->fast_auto_windows = set_windows < 8 ? 8 : (set_windows > 2048 ? 2048 : set_windows);
    return c->fast_auto_windows;
}

// MCRAT_HIP_MODE_FAST for the lists of a rank pool, one launch: list r (open[r] != 0) runs its frame of remaining_time[r] with its own seed
// and stream and list-local slot numbers in its keys -- bit for bit what mcrat_hip_propagate_frame_mode(view r, ..., seeds[r], FAST, ...) gives
extern "C" int mcrat_hip_pool_propagate_frames_fast(mcrat_hip_ctx *c, const int *open, const uint64_t *seeds, const double *time_now,
                                                    const double *remaining_time, int fast_windows, mcrat_hip_frame_stats *stats)
{
    if (!c || !open || !seeds || !time_now || !remaining_time) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "pool_propagate_frames_fast")) return rc_;
    if (c->d_pool_tapes) { c->last_error = "the pool holds tapes of uniforms (mcrat_hip_pool_set_rng_tapes): FAST mode has no tape build"; return MCRAT_HIP_ESTATE; }
    int rc = fast_refusals(c);
    if (rc) return rc;
    const int R = c->n_ranks;
    std::vector<double> rem((size_t)R, 0.0);
    for (int r = 0; r < R; ++r) {
        mcrat_hip_ctx *v = c->views[r];
        c->h_desc[r] = RankDesc{};
        if (!open[r]) continue;
        if (!v || !v->have_photons) { c->last_error = "pool_propagate_frames_fast: a list that does not exist was asked to run a frame"; return MCRAT_HIP_ESTATE; }
        if ((rc = flush_pending(v))) return rc;
        c->h_desc[r].len = v->ph.n; c->h_desc[r].stream = v->key.stream; c->h_desc[r].seed = seeds[r];
        rem[(size_t)r] = remaining_time[r] > 0 ? remaining_time[r] : 0.0;
    }
    std::vector<int> win((size_t)R, 8);                      // every list its own cadence (fast_cadence_learn): as its view run alone would have
    for (int r = 0; r < R; ++r)
        if (open[r]) win[(size_t)r] = fast_cadence(c->views[r], fast_windows);
    const size_t bytes = (sizeof(FastCounts) + sizeof(double) + sizeof(int)) * (size_t)R;
    if ((rc = ensure_aos(c, bytes + 64))) return rc;
    FastCounts *d_cnt = static_cast<FastCounts *>(c->aos_buf);
    double *d_rem = reinterpret_cast<double *>(d_cnt + R);
    int *d_win = reinterpret_cast<int *>(d_rem + R);
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(FastCounts) * (size_t)R, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rem, rem.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_win, win.data(), sizeof(int) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    const FastLists lists{c->rank_stride, c->d_desc, d_rem, d_win};
    HIPCHK(c, launch_fast_frame(c->kc, c->ph, c->hy, c->key, 0.0, 8, 1 << 22, d_cnt, lists, c->stream));
    std::vector<FastCounts> cnt((size_t)R);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(FastCounts) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->frame_open = false;
    unsigned long long unfinished = 0, scatterings = 0;
    long long photons = 0;
    for (int r = 0; r < R; ++r) {
        if (!open[r]) continue;
        mcrat_hip_ctx *v = c->views[r];
        v->frame_open = false; v->pending_applied = false; v->rank_current = true;
        unfinished += cnt[(size_t)r].unfinished;
        scatterings += cnt[(size_t)r].scatterings; photons += v->ph.n;
        if (rem[(size_t)r] > 0) fast_cadence_learn(v, cnt[(size_t)r].scatterings, v->ph.n);
        if (stats) fast_stats(cnt[(size_t)r], time_now[r] + rem[(size_t)r], &stats[r]);
    }
    (void)scatterings; (void)photons;
    if (unfinished) { c->last_error = "FAST mode: photons left with frame time after 2^22 passes (an optical depth of infinity?)"; return MCRAT_HIP_ESTATE; }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_propagate_frame_mode(mcrat_hip_ctx *c, double *time_now, double remaining_time, uint64_t seed, int mode, int fast_windows,
                                              mcrat_hip_frame_stats *stats)
{
    if (!c || !time_now) return MCRAT_HIP_EINVAL;
    if (mode == MCRAT_HIP_MODE_EXACT) return mcrat_hip_propagate_frame(c, time_now, remaining_time, seed, stats);
    if (mode != MCRAT_HIP_MODE_FAST) return MCRAT_HIP_EINVAL;
    int rc = fast_refusals(c);
    if (rc) return rc;
    if (c->is_pool) {                                                  // every list that holds photons, the same seed and frame time
        const int R = c->n_ranks;
        std::vector<int> open((size_t)R, 0);
        std::vector<uint64_t> seeds((size_t)R, seed);
        std::vector<double> t((size_t)R, *time_now), rem((size_t)R, remaining_time);
        std::vector<mcrat_hip_frame_stats> per((size_t)R);
        bool any = false;
        for (int r = 0; r < R; ++r) { open[(size_t)r] = c->views[r] && c->views[r]->have_photons; any = any || open[(size_t)r]; }
        if (!any) return MCRAT_HIP_ESTATE;
        if ((rc = mcrat_hip_pool_propagate_frames_fast(c, open.data(), seeds.data(), t.data(), rem.data(), fast_windows, per.data()))) return rc;
        if (remaining_time > 0) *time_now += remaining_time;
        if (stats) {
            FastCounts sum{};
            for (int r = 0; r < R; ++r) {
                if (!open[(size_t)r]) continue;
                const mcrat_hip_frame_stats &q = per[(size_t)r];
                sum.passes = std::max<unsigned long long>(sum.passes, (unsigned long long)q.iterations);
                sum.photon_steps += (unsigned long long)q.photon_steps; sum.scatterings += (unsigned long long)q.frame_scatt_cnt;
                sum.kn_rejections += (unsigned long long)q.kn_rejections; sum.relocated += (unsigned long long)q.num_photons_find_new_element;
                sum.not_found += (unsigned long long)q.not_found;
            }
            fast_stats(sum, *time_now, stats);
        }
        return MCRAT_HIP_OK;
    }
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    if (c->frame_open && c->n_ranks == 0 && (rc = flush_pending(c))) return rc;       // what a list-mode run still owes the photons
    if (!c->d_fast) HIPCHK(c, hipMalloc(&c->d_fast, sizeof(FastCounts)));
    HIPCHK(c, hipMemsetAsync(c->d_fast, 0, sizeof(FastCounts), c->stream));
    RngKey key = c->key;
    key.seed = seed;
    FastCounts fc{};
    if (remaining_time > 0) {
        HIPCHK(c, launch_fast_frame(c->kc, c->ph, c->hy, key, remaining_time, fast_cadence(c, fast_windows), 1 << 22,
                                    static_cast<FastCounts *>(c->d_fast), FastLists{0, nullptr, nullptr, nullptr}, c->stream));
        HIPCHK(c, hipMemcpyAsync(&fc, c->d_fast, sizeof fc, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (remaining_time > 0) fast_cadence_learn(c, fc.scatterings, c->ph.n);
    c->frame_open = false;
    c->pending_applied = false;
    if (c->parent) c->rank_current = true;
    if (fc.unfinished) { c->last_error = "FAST mode: photons left with frame time after 2^22 passes (an optical depth of infinity?)"; return MCRAT_HIP_ESTATE; }
    if (remaining_time > 0) *time_now += remaining_time;
    if (stats) fast_stats(fc, *time_now, stats);
    return MCRAT_HIP_OK;
}

// ---- the hook's state of a list (CsFrame, launch.hpp) as the host keeps it through a scatter frame: what the one-list frame and the pool's frame share
// at the start of a frame; carried: main()'s scatt_cyclosynch_num_ph of the frame before (mcrat.c:873,921)
static CsFrame cs_frame_begin(int max_photons, int carried) { CsFrame f{}; f.max_photons = max_photons; f.last_iteration = ~0ull; f.scatt_num = carried; return f; }
// a parked list goes on: the loop's `done` gets back what the pass left (the hook saved it).  The host's copies here; send_done and a copy of the
// CsFrame take them to the device.
static void cs_frame_release(CsFrame &f, LoopState *h_state) { f.halt = 0; h_state->done = f.saved_done; }
static hipError_t send_done(const LoopState *h_state, LoopState *d_state, hipStream_t stream)
{
    return hipMemcpyAsync(reinterpret_cast<char *>(d_state) + offsetof(LoopState, done), &h_state->done, sizeof(int), hipMemcpyHostToDevice, stream);
}
// the list was rebinned inside the loop (:797-808): the rebinning's two counters replace the frame's
static void cs_frame_rebinned(CsFrame &f, mcrat_hip_cyclosynch_counts &cnt, int &emit_base, int num_cyclosynch_ph_emit, int scatt_cyclosynch_num_ph)
{
    cnt.rebins += 1;
    emit_base = num_cyclosynch_ph_emit; f.emitted = 0;       // num_cyclosynch_ph_emit = emit_base + replacements since (the rebinning overwrites it)
    f.scatt_num = scatt_cyclosynch_num_ph;
}
// the loop is over: the frame's counters from the hook's state
static void cs_frame_close(const CsFrame &f, int emit_base, mcrat_hip_cyclosynch_counts &cnt)
{
    cnt.num_cyclosynch_ph_emit = emit_base + f.emitted; cnt.scatt_cyclosynch_num_ph = f.scatt_num; cnt.n_comptonized = f.n_comptonized;
}
// the end of the frame, mcrat.c:853-878: rebin a list that holds more comptonised photons than max_photons, then absorb if anything was emitted
static bool cs_end_rebin_due(int emit_pool, const mcrat_hip_cyclosynch_counts &cnt, int max_photons) { return emit_pool && cnt.scatt_cyclosynch_num_ph > max_photons; }
static bool cs_end_absorb_due(int emit_pool, const mcrat_hip_cyclosynch_counts &cnt) { return emit_pool && cnt.num_cyclosynch_ph_emit > 0; }

// The scatter-frame body of main() with CYCLOSYNCHROTRON_SWITCH on (mcrat.c:706-878, between getHydroData and saveCheckpoint): pool
// emission, the loop with the replacement of scattered pool photons (:786-795) and the rebinning trigger (:797-808), the rebinning
// and absorption at the end of the frame (:853-878).  The hook needs the list current after every pass, so a pass here is
// step + event + flush + cs_replace; the hook keeps the frame's counters on the device and parks the loop when it needs the host
// (list growth, the rebinning), so the host reads back once per batch of passes (CsFrame, launch.hpp).
extern "C" int mcrat_hip_scatter_frame_cyclosynch(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, double *time_now, double remaining_time, uint64_t seed,
                                                  double r_inj, double ph_weight_suggest, int max_photons, double theta_min, double theta_max, double fps,
                                                  int emit_pool, long long max_iterations, mcrat_hip_frame_stats *stats, mcrat_hip_cyclosynch_counts *cnt)
{
    if (!c || !cs || !time_now || !cnt || cs->b_field_calc < 0 || cs->b_field_calc > 2 || max_photons <= 0) return MCRAT_HIP_EINVAL;
    if (!c->cfg.cyclosynchrotron_switch) { c->last_error = "the context was created with cyclosynchrotron_switch = 0"; return MCRAT_HIP_ESTATE; }
    if (c->n_ranks > 0 || c->sc_world > 0) return MCRAT_HIP_ESTATE;
    if (!c->have_hydro || !c->hcol_buf || !c->have_photons) return MCRAT_HIP_ESTATE;
    const int carried = cnt->scatt_cyclosynch_num_ph;        // main()'s counter lives across the scatter frames of an injection (mcrat.c:873,921)
    memset(cnt, 0, sizeof *cnt);
    int rc;
    if (emit_pool) {                                                                              // :727-744
        int n = 0, bad = 0;
        double w = 0;
        if ((rc = mcrat_hip_emit_cyclosynch_pool(c, cs, r_inj, ph_weight_suggest, max_photons, theta_min, theta_max, fps, seed, &n, &w, &bad))) return rc;
        cnt->num_cyclosynch_ph_emit = n;
        cnt->pool_weight = w;
        cnt->integrals_not_converged = bad;
    }
    if ((rc = mcrat_hip_begin_frame(c, seed, *time_now, remaining_time))) return rc;
    const CsEmitParams p = cs_emit_params(c, cs);
    if (!c->d_cs_hook) HIPCHK(c, hipMalloc((void **)&c->d_cs_hook, sizeof(CsFrame)));
    CsFrame *d_cf = static_cast<CsFrame *>(c->d_cs_hook);
    CsFrame cf = cs_frame_begin(max_photons, carried);
    HIPCHK(c, hipMemcpyAsync(d_cf, &cf, sizeof cf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                                  // cf is on the stack
    int emit_base = cnt->num_cyclosynch_ph_emit;
    const long long per_sync = 32;                 // passes queued per read-back; a parked loop makes the rest of a batch no-ops
    while (!c->h_state->done && (max_iterations <= 0 || c->h_state->iterations < max_iterations)) {   // :761-851
        long long batch = per_sync;
        if (max_iterations > 0 && batch > max_iterations - c->h_state->iterations) batch = max_iterations - c->h_state->iterations;
        auto one_pass = [&](bool force) -> int {
            HIPCHK(c, launch_step(c->kc, force, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream));
            HIPCHK(c, launch_event(c->kc, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream));
            HIPCHK(c, launch_flush(c->ph, c->d_state, c->step_blocks, c->stream));
            HIPCHK(c, launch_cs_replace(p, c->hy, c->hcol, c->key, c->d_state, c->ph, d_cf, 0, c->stream));
            return MCRAT_HIP_OK;
        };
        for (long long b = 0; b < batch; ++b) {       // (a batch as one hipGraph launch was measured: 33.7 against 34.6 us per pass, not kept)
            if ((rc = one_pass(c->find_switch != 0))) return rc;
            c->find_switch = 0;
        }
        HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&cf, d_cf, sizeof cf, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        while (cf.halt) {                          // the loop is parked: do what the hook asked for, then let it go on
            const int why = cf.halt;
            cs_frame_release(cf, c->h_state);
            HIPCHK(c, send_done(c->h_state, c->d_state, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (why == CS_HALT_GROW) {                                                            // photons.c:112-121: the list doubles
                if (c->ph.n > 0x3fffffff) { c->last_error = "photon list too long to double"; return MCRAT_HIP_ENOMEM; }
                HIPCHK(c, hipMemcpyAsync(d_cf, &cf, sizeof cf, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if ((rc = grow_photons(c, 2 * c->ph.n))) return rc;
                HIPCHK(c, launch_cs_replace(p, c->hy, c->hcol, c->key, c->d_state, c->ph, d_cf, 1, c->stream));
                HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(&cf, d_cf, sizeof cf, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (cf.halt == CS_HALT_GROW) { c->last_error = "the replacement of a scattered pool photon failed after the list was doubled"; return MCRAT_HIP_ENOMEM; }
            } else {                                                                              // :797-808
                int empty = 0, emit_total = emit_base + cf.emitted, scatt = cf.scatt_num;
                rc = mcrat_hip_rebin_cyclosynch(c, cs, max_photons, &empty, &emit_total, &scatt);
                if (rc == MCRAT_HIP_OK) cs_frame_rebinned(cf, *cnt, emit_base, emit_total, scatt);
                else if (rc != MCRAT_HIP_EREFUSED) return rc;      // EREFUSED: one of the reference's refusals, the list is as it was
                HIPCHK(c, hipMemcpyAsync(d_cf, &cf, sizeof cf, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
        }
    }
    cs_frame_close(cf, emit_base, *cnt);
    c->pending_applied = false;
    if (cs_end_rebin_due(emit_pool, *cnt, max_photons)) {                                         // :853-878
        int empty = 0;
        rc = mcrat_hip_rebin_cyclosynch(c, cs, max_photons, &empty, &cnt->num_cyclosynch_ph_emit, &cnt->scatt_cyclosynch_num_ph);
        if (rc == MCRAT_HIP_OK) cnt->rebins += 1;
        else if (rc != MCRAT_HIP_EREFUSED) return rc;
    }
    if (cs_end_absorb_due(emit_pool, *cnt)) {
        double w = 0;
        if ((rc = mcrat_hip_absorb_cyclosynch(c, cs, &cnt->frame_abs_cnt, &cnt->scatt_cyclosynch_num_ph, &w))) return rc;
        cnt->n_comptonized -= w;
    }
    HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *time_now = c->h_state->time_now;
    fill_stats(c, stats);
    return MCRAT_HIP_OK;
}

// One call of mcrat_hip_pool_scatter_frames_cyclosynch: its arguments, what it keeps per list, and what its steps hand on.
struct PoolCsFrames {
    mcrat_hip_ctx *c;
    const mcrat_hip_cyclosynch *cs;
    int max_photons, R;
    double fps;
    const mcrat_hip_pool_cs_list *lists;
    mcrat_hip_frame_stats *stats;                // may be null
    mcrat_hip_cyclosynch_counts *counts;
    bool hook_kernel;                            // MCRAT_HIP_CS_HOOK_KERNEL=1: the hook as a kernel between two launches of the loop (the first form, kept for the A/B)
    // per list: what mcrat_hip_pool_begin_frames takes; cs with the list's own frame numbers; the counter main() carries from the previous frame
    // (mcrat.c:873,921); num_cyclosynch_ph_emit = emit_base + replacements since (the rebinning overwrites it)
    std::vector<int> open, carried, emit_base;
    std::vector<uint64_t> seeds;
    std::vector<double> t_now, t_rem;
    std::vector<mcrat_hip_cyclosynch> csr;
    std::vector<CsFrame> cf;                     // the hooks' state, the host's copy
    CsFrame *d_cf = nullptr;                     // ... and the device's (the context's d_cs_hook)
    CsEmitParams p;                              // what the hook is given
    bool emits(int r) const { return open[(size_t)r] && lists[r].emit_pool; }
};

// photonEmitCyclosynch (mc_cyclosynch.c:1219-1460, inject_single_switch = 0) for the lists of a rank pool that ask for it: the emission
// shell of each group of lists that share one (same radii and angles) is found and integrated once, then one workgroup per list runs the
// list's weight loop and places its photons (inject.hip).  A list with more photons than that kernel's tables hold takes the one-list
// path (mcrat_hip_emit_cyclosynch_pool on its view); both give the same photons.
static int pool_emit_cyclosynch(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    const mcrat_hip_pool_cs_list *lists = F.lists;
    const int R = F.R, M = c->hy.M;
    std::vector<Region> shells((size_t)R);                  // the lists grouped by their shell
    int n_shells = 0;
    std::vector<CsPoolEmit> pe((size_t)R);
    bool any = false;
    int rc;
    for (int r = 0; r < R; ++r) {
        pe[(size_t)r] = CsPoolEmit{};
        c->h_desc[r] = RankDesc{};
        if (!lists[r].open || !lists[r].emit_pool) continue;
        if (!(lists[r].ph_weight_suggest > 0)) return MCRAT_HIP_EINVAL;
        mcrat_hip_ctx *v = c->views[r];
        if ((rc = flush_pending(v))) return rc;
        const RadialRange sh = emit_shell_radii(lists[r].r_inj, F.csr[(size_t)r].scatt_frame_number, F.csr[(size_t)r].inj_frame_number, F.fps);
        CsPoolEmit &e = pe[(size_t)r];
        e.open = 1; e.group = region_group(shells.data(), &n_shells, Region{sh.rmin, sh.rmax, lists[r].theta_min, lists[r].theta_max, 0});
        e.seed = lists[r].seed; e.weight_in = lists[r].ph_weight_suggest; e.max_photons = F.cs->rebin_e_perc * F.max_photons;
        c->h_desc[r].len = v->ph.n; c->h_desc[r].stream = v->key.stream; c->h_desc[r].seed = lists[r].seed;
        any = true;
    }
    if (!any) return MCRAT_HIP_OK;
    if ((rc = ensure_counts(c, (size_t)M + 8))) return rc;
    std::vector<unsigned> bad((size_t)n_shells, 0);
    {                                                       // (the temporaries go before the lists are looked at: a list may take the one-list path below)
        const size_t scan_ints = (size_t)M + 1 + grid_scan_scratch_ints(M);
        DeviceTemp<int> d_start;
        DeviceTemp<CsPoolEmit> d_pe;
        DeviceTemp<CsShellCell> d_shell;
        DeviceTemp<unsigned> d_bad;
        if (d_start.alloc(scan_ints) != hipSuccess || d_pe.alloc((size_t)R) != hipSuccess || d_bad.alloc(1) != hipSuccess) return MCRAT_HIP_ENOMEM;
        if (hipMemcpyAsync(d_pe, pe.data(), sizeof(CsPoolEmit) * (size_t)R, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyHostToDevice, c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
        CsEmitParams p = cs_emit_params(c, F.cs);
        for (int g = 0; g < n_shells; ++g) {
            emit_into(p, shells[(size_t)g]);
            int n_shell = 0;
            if ((rc = pool_region_cells(c, p, d_shell, &n_shell,
                                        [&] { return launch_region_write(p, c->hy, c->hcol, c->grid_count, n_shell, d_start, d_start + M + 1, d_shell, d_bad, c->stream); })))
                return rc;
            if (launch_cs_emit_pool(p, c->hy, c->hcol, c->ph, c->rank_stride, R, c->d_desc, d_shell, n_shell, d_pe, g, c->stream) != hipSuccess ||
                hipMemcpyAsync(&bad[g], d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) { c->last_error = "cyclo-synchrotron emission of the pool's lists failed"; return MCRAT_HIP_EHIP; }
        }
        if (hipMemcpyAsync(pe.data(), d_pe, sizeof(CsPoolEmit) * (size_t)R, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->h_desc, c->d_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return MCRAT_HIP_EHIP;
    }
    for (int r = 0; r < R; ++r) {
        const CsPoolEmit &e = pe[(size_t)r];
        if (!e.open) continue;
        mcrat_hip_ctx *v = c->views[r];
        int n = e.n_emit, nbad = (int)bad[(size_t)e.group];
        double w = e.weight_out;
        if (nbad > 0) return emit_not_converged(c, (unsigned)nbad);       // (as mcrat_hip_emit_cyclosynch_pool)
        switch (e.error) {
        case 0:
            v->ph.n = c->h_desc[r].len;                                                           // the list may have grown inside its window
            if (n > 0) { v->frame_open = false; drop_graph(v); }
            break;
        case 4:                                                                                   // more photons than the kernel's tables hold
            if ((rc = mcrat_hip_emit_cyclosynch_pool(v, &F.csr[(size_t)r], lists[r].r_inj, lists[r].ph_weight_suggest, F.max_photons, lists[r].theta_min,
                                                     lists[r].theta_max, F.fps, lists[r].seed, &n, &w, &nbad))) { c->last_error = v->last_error; return rc; }
            break;
        case 1: c->last_error = list_refusal_text(EMIT_NO_WEIGHT); return MCRAT_HIP_EINVAL;
        case 2: c->last_error = list_refusal_text(EMIT_NO_NULL_SLOTS); return MCRAT_HIP_EINVAL;
        default: c->last_error = "the list is longer than the pool's slots per rank (mcrat_hip_pool_create)"; return MCRAT_HIP_ENOMEM;
        }
        F.counts[r].num_cyclosynch_ph_emit = n;
        F.counts[r].pool_weight = w;
        F.counts[r].integrals_not_converged = nbad;
        F.emit_base[(size_t)r] = n;
    }
    return MCRAT_HIP_OK;
}

// the rebinning of the pool's lists `ids`: all at once (pool_rebin_lists), or -- MCRAT_HIP_POOL_REBIN_EACH=1, the round-2 path kept for the A/B and
// the equality test -- list by list through the views
static int pool_rebin(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, int max_photons, const std::vector<int> &ids, std::vector<PoolRebinResult> &res)
{
    if (!env_flag("MCRAT_HIP_POOL_REBIN_EACH")) return pool_rebin_lists(c, cs, max_photons, ids, res);
    res.assign(ids.size(), PoolRebinResult{MCRAT_HIP_OK, 0, 0, 0});
    for (size_t j = 0; j < ids.size(); ++j) {
        mcrat_hip_ctx *v = c->views[ids[j]];
        const int rc = mcrat_hip_rebin_cyclosynch(v, cs, max_photons, &res[j].empty_bins, &res[j].num_cyclosynch_ph_emit, &res[j].scatt_cyclosynch_num_ph);
        res[j].rc = rc;
        if (rc != MCRAT_HIP_OK && rc != MCRAT_HIP_EREFUSED) { c->last_error = v->last_error; return rc; }
    }
    return MCRAT_HIP_OK;
}

// ---- the steps of mcrat_hip_pool_scatter_frames_cyclosynch, in the order it takes them
// 1. the open lists and their arguments; every list's counters start from zero
static int pcs_collect(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    const size_t R = (size_t)F.R;
    F.open.assign(R, 0); F.emit_base.assign(R, 0); F.carried.assign(R, 0); F.seeds.assign(R, 0);
    F.t_now.assign(R, 0.0); F.t_rem.assign(R, 0.0); F.csr.assign(R, *F.cs);
    for (int r = 0; r < F.R; ++r) {
        F.carried[(size_t)r] = F.counts[r].scatt_cyclosynch_num_ph;
        memset(&F.counts[r], 0, sizeof F.counts[r]);
        const mcrat_hip_pool_cs_list &l = F.lists[r];
        if (!l.open) continue;
        mcrat_hip_ctx *v = c->views[r];
        if (!v || !v->have_photons) { c->last_error = "pool_scatter_frames_cyclosynch: an open list does not exist"; return MCRAT_HIP_ESTATE; }
        F.open[(size_t)r] = 1;
        F.seeds[(size_t)r] = l.seed; F.t_now[(size_t)r] = l.time_now; F.t_rem[(size_t)r] = l.remaining_time;
        F.csr[(size_t)r].scatt_frame_number = l.scatt_frame_number;
        F.csr[(size_t)r].inj_frame_number = l.inj_frame_number;
    }
    return MCRAT_HIP_OK;
}
// 4. the hooks' state, one CsFrame per list, the lists' descriptions, and what the hook is given
static int pcs_upload_hooks(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    const size_t R = (size_t)F.R;
    if (c->d_cs_hook) { HIPCHK(c, hipFree(c->d_cs_hook)); c->d_cs_hook = nullptr; }
    HIPCHK(c, hipMalloc((void **)&c->d_cs_hook, sizeof(CsFrame) * R));
    F.d_cf = static_cast<CsFrame *>(c->d_cs_hook);
    F.cf.resize(R);
    for (size_t r = 0; r < R; ++r) F.cf[r] = cs_frame_begin(F.max_photons, F.carried[r]);
    HIPCHK(c, hipMemcpyAsync(F.d_cf, F.cf.data(), sizeof(CsFrame) * R, hipMemcpyHostToDevice, c->stream));
    int rc = pool_describe(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    F.p = cs_emit_params(c, F.cs);
    if (!c->d_cs_args) HIPCHK(c, hipMalloc(&c->d_cs_args, sizeof(CsHookArgs)));
    CsHookArgs ha;
    ha.p = F.p; ha.h = c->hcol;
    HIPCHK(c, hipMemcpyAsync(c->d_cs_args, &ha, sizeof ha, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}
// 5. threads per list (rank_form_plan.hpp, cs_rank_block_rule)
static void pcs_choose_block(PoolCsFrames &F)
{
    const RankBlock b = cs_rank_block_rule(F.R, device_cus(F.c), F.hook_kernel, rank_env());
    F.c->rank_block = b.threads; F.c->rank_fuse = b.fuse;
}
// 6. the loop.  The hook runs inside rank_loop_kernel (its CSH build: cs_hook_body right after the pass, the list goes on in the same launch); with
// hook_kernel the lists park after such a pass instead and cs_replace_pool_kernel runs it between two launches.  Either way a list only stays
// parked for the host when it has to be rebinned (:797-808): all parked lists in the same two launches, then they go on.
static int pcs_loop(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    const int R = F.R;
    int rc;
    const int pairs_per_sync = F.hook_kernel ? 8 : 2;
    RankLaunch rl = rank_launch_of(c, c->d_desc, 4096);
    rl.longest_list = RANK_COLUMNS_GLOBAL;           // (lists that change length: their columns stay in HBM/L2)
    rl.cs = F.d_cf;
    rl.hook = F.hook_kernel ? nullptr : static_cast<const CsHookArgs *>(c->d_cs_args);
    for (;;) {
        rc = profiled(c, pairs_per_sync, [&]() -> int {         // the loop's launches between events (bench.py: cfg5's loop-only roofline)
            for (int k = 0; k < pairs_per_sync; ++k) {
                HIPCHK(c, launch_rank_loop(c->kc, c->ph, c->hy, c->d_rstates, c->key, rl, c->stream));
                if (F.hook_kernel) HIPCHK(c, launch_cs_replace_pool(F.p, c->hy, c->hcol, c->d_rstates, c->ph, c->rank_stride, R, c->d_desc, F.d_cf, c->stream));
            }
            return MCRAT_HIP_OK;
        });
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->h_rstates, c->d_rstates, sizeof(LoopState) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(F.cf.data(), F.d_cf, sizeof(CsFrame) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_desc, c->d_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int> parked;                                                                  // lists waiting for rebinCyclosynchCompPhotons
        for (int r = 0; r < R; ++r) {
            if (!F.open[(size_t)r]) continue;
            c->views[r]->ph.n = c->h_desc[r].len;                                                 // the list may have doubled in the hook
            if (F.cf[(size_t)r].halt == CS_HALT_GROW) {
                c->last_error = "a cyclo-synchrotron list outgrew the pool's slots per rank (mcrat_hip_pool_create: allow for the doublings)";
                return MCRAT_HIP_ENOMEM;
            }
            if (F.cf[(size_t)r].halt == CS_HALT_REBIN) parked.push_back(r);
        }
        if (!parked.empty()) {
            std::vector<PoolRebinResult> res;
            if ((rc = pool_rebin(c, F.cs, F.max_photons, parked, res))) return rc;
            for (size_t j = 0; j < parked.size(); ++j) {
                const int r = parked[j];
                CsFrame &f = F.cf[(size_t)r];
                if (res[j].rc == MCRAT_HIP_OK) cs_frame_rebinned(f, F.counts[r], F.emit_base[(size_t)r], res[j].num_cyclosynch_ph_emit, res[j].scatt_cyclosynch_num_ph);
                cs_frame_release(f, &c->h_rstates[r]);
                HIPCHK(c, hipMemcpyAsync(F.d_cf + r, &f, sizeof f, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, send_done(&c->h_rstates[r], c->d_rstates + r, c->stream));
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        bool all_done = true;
        for (int r = 0; r < R; ++r)
            if (F.open[(size_t)r] && c->h_rstates[r].done != LOOP_DONE) all_done = false;
        if (all_done) return MCRAT_HIP_OK;
    }
}
// 7. the frames' counters from the hooks' state; the lists are current
static void pcs_close_counters(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    for (int r = 0; r < F.R; ++r) {
        if (!F.open[(size_t)r]) continue;
        mcrat_hip_ctx *v = c->views[r];
        cs_frame_close(F.cf[(size_t)r], F.emit_base[(size_t)r], F.counts[r]);
        v->pending_applied = false;
        v->rank_current = true;
        if (F.stats) state_to_stats(c->h_rstates[r], v->ph.n, &F.stats[r]);
    }
}
// 8. :853-878, the lists over max_photons all at once
static int pcs_end_rebin(PoolCsFrames &F)
{
    std::vector<int> over;
    for (int r = 0; r < F.R; ++r)
        if (cs_end_rebin_due(F.emits(r), F.counts[r], F.max_photons)) over.push_back(r);
    std::vector<PoolRebinResult> res;
    int rc = pool_rebin(F.c, F.cs, F.max_photons, over, res);
    if (rc) return rc;
    for (size_t j = 0; j < over.size(); ++j) {
        if (res[j].rc != MCRAT_HIP_OK) continue;
        const int r = over[j];
        F.counts[r].rebins += 1;
        F.counts[r].num_cyclosynch_ph_emit = res[j].num_cyclosynch_ph_emit;
        F.counts[r].scatt_cyclosynch_num_ph = res[j].scatt_cyclosynch_num_ph;
    }
    return MCRAT_HIP_OK;
}
// 9. phAbsCyclosynch of every list that emitted, one launch
static int pcs_absorb(PoolCsFrames &F)
{
    mcrat_hip_ctx *c = F.c;
    const int R = F.R;
    int rc;
    std::vector<int> absorb((size_t)R, 0);
    bool any_absorb = false;
    for (int r = 0; r < R; ++r)
        if (cs_end_absorb_due(F.emits(r), F.counts[r])) { absorb[(size_t)r] = 1; any_absorb = true; }
    if (!any_absorb) return MCRAT_HIP_OK;
    for (int r = 0; r < R; ++r)
        if (absorb[(size_t)r] && (rc = flush_pending(c->views[r]))) return rc;
    for (int r = 0; r < R; ++r) { c->h_desc[r].len = F.open[(size_t)r] ? c->views[r]->ph.n : 0; }
    const size_t bytes = (sizeof(CsAbsPartial) + sizeof(int)) * (size_t)R;
    if ((rc = ensure_aos(c, bytes + 64))) return rc;
    CsAbsPartial *d_part = static_cast<CsAbsPartial *>(c->aos_buf);
    int *d_sel = reinterpret_cast<int *>(d_part + R);
    std::vector<CsAbsPartial> part((size_t)R);
    HIPCHK(c, hipMemcpyAsync(c->d_desc, c->h_desc, sizeof(RankDesc) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_sel, absorb.data(), sizeof(int) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    CsParams ap{c->kc.dimensions, F.cs->b_field_calc, F.cs->epsilon_b};
    HIPCHK(c, launch_cs_absorb_pool(ap, c->ph, c->rank_stride, R, c->d_desc, d_sel, c->hy.temp, c->hcol, d_part, c->stream));
    HIPCHK(c, hipMemcpyAsync(part.data(), d_part, sizeof(CsAbsPartial) * (size_t)R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < R; ++r) {
        if (!absorb[(size_t)r]) continue;
        F.counts[r].frame_abs_cnt = (int)part[(size_t)r].abs_count;
        F.counts[r].scatt_cyclosynch_num_ph = (int)part[(size_t)r].scatt_count;
        F.counts[r].n_comptonized -= part[(size_t)r].abs_weight;
        drop_graph(c->views[r]);
    }
    return MCRAT_HIP_OK;
}

// The scatter frame of mcrat.c:706-878 with CYCLOSYNCHROTRON_SWITCH on for the lists of a rank pool: what mcrat_hip_scatter_frame_cyclosynch
// does for one list, for every open list -- the loop of all of them in the same launches.  rank_loop_kernel (its CSH build) runs every list
// and, after a pass the hook of :786-808 must look at (photonEvent reported a pool photon; a thousand scatterings are full), the hook itself:
// it converts and replaces the pool photon (doubling the list inside its window of the pool when it has no null slot left) and evaluates
// the rebinning trigger; the list goes on in the same launch.  Only the rebinning itself parks a list for the host (pool_rebin).
// (First form, MCRAT_HIP_CS_HOOK_KERNEL=1: the list parks after every such pass and cs_replace_pool_kernel, one workgroup per parked list,
// runs the hook between two launches of the loop, 8 pairs per read-back; no 64-thread lists.)
extern "C" int mcrat_hip_pool_scatter_frames_cyclosynch(mcrat_hip_ctx *c, const mcrat_hip_cyclosynch *cs, int max_photons, double fps,
                                                        const mcrat_hip_pool_cs_list *lists, mcrat_hip_frame_stats *stats,
                                                        mcrat_hip_cyclosynch_counts *counts)
{
    if (!c || !cs || !lists || !counts || cs->b_field_calc < 0 || cs->b_field_calc > 2 || max_photons <= 0 || !(fps > 0)) return MCRAT_HIP_EINVAL;
    if (!c->is_pool) return MCRAT_HIP_ESTATE;
    if (int rc_ = capture_refuses(c, "pool_scatter_frames_cyclosynch")) return rc_;
    if (!c->cfg.cyclosynchrotron_switch) { c->last_error = "the pool was created with cyclosynchrotron_switch = 0"; return MCRAT_HIP_ESTATE; }
    if (c->d_pool_tapes) { c->last_error = "the pool holds tapes of uniforms (mcrat_hip_pool_set_rng_tapes): the cyclo-synchrotron hook has no tape build"; return MCRAT_HIP_ESTATE; }
    if (!c->have_hydro || !c->hcol_buf) return MCRAT_HIP_ESTATE;
    PoolCsFrames F{};
    F.c = c; F.cs = cs; F.max_photons = max_photons; F.R = c->n_ranks; F.fps = fps; F.lists = lists; F.stats = stats; F.counts = counts;
    F.hook_kernel = env_flag("MCRAT_HIP_CS_HOOK_KERNEL");
    int rc;
    if ((rc = pcs_collect(F))) return rc;
    if ((rc = pool_emit_cyclosynch(F))) return rc;                                                                     // :727-744
    if ((rc = mcrat_hip_pool_begin_frames(c, F.open.data(), F.seeds.data(), F.t_now.data(), F.t_rem.data()))) return rc;
    if ((rc = pcs_upload_hooks(F))) return rc;
    pcs_choose_block(F);
    if ((rc = pcs_loop(F))) return rc;                                                                                 // :761-851
    pcs_close_counters(F);
    if ((rc = pcs_end_rebin(F))) return rc;                                                                            // :853-878
    return pcs_absorb(F);
}

extern "C" int mcrat_hip_step_locate_sample(mcrat_hip_ctx *c, int find_nearest_block_switch)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->frame_open || c->n_ranks > 0) return MCRAT_HIP_ESTATE;
    HIPCHK(c, launch_step(c->kc, find_nearest_block_switch != 0, c->ph, c->hy, c->d_state, c->key, c->partials, c->step_blocks, c->shortlist, c->stream));
    c->find_switch = 0;
    c->pending_applied = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_frame_statistics(mcrat_hip_ctx *c, mcrat_hip_frame_stats *stats)
{
    if (!c || !stats) return MCRAT_HIP_EINVAL;
    if (!c->frame_open || c->n_ranks > 0) return MCRAT_HIP_ESTATE;
    HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fill_stats(c, stats);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_update_photon_position(mcrat_hip_ctx *c, double t)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    int rc;
    if (c->frame_open && c->n_ranks == 0 && (rc = flush_pending(c))) return rc;      // what the loop still owes the photons
    c->pending_applied = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int nseg = 1, skip = -1;
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(c->d_state) + offsetof(LoopState, seg), &t, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(c->d_state) + offsetof(LoopState, nseg), &nseg, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(c->d_state) + offsetof(LoopState, skip_idx), &skip, sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, launch_flush(c->ph, c->d_state, c->step_blocks, c->stream));          // r += (p/p0) c t, mclib.c:1067-1095
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_step_event(mcrat_hip_ctx *c, mcrat_hip_frame_stats *stats)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->frame_open || c->n_ranks > 0) return MCRAT_HIP_ESTATE;
    HIPCHK(c, launch_event_of(c));
    c->pending_applied = false;
    HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fill_stats(c, stats);
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- shared clock
extern "C" size_t mcrat_hip_shared_clock_bytes_per_rank(void) { return sizeof(ScProposal); }

extern "C" int mcrat_hip_shared_clock_attach(mcrat_hip_ctx *c, int world, int rank, long long slot_base, void *send, void *recv)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (world < 1 || world > SC_MAX_WORLD || rank < 0 || rank >= world) return MCRAT_HIP_EINVAL;
    if (slot_base < 0 || (slot_base & 1) || slot_base > 0xffffffffll - 0x7fffffffll) {
        c->last_error = "slot_base must be even, non-negative and leave room for 2^31 slots below 2^32";
        return MCRAT_HIP_EINVAL;
    }
    if (c->n_ranks > 0 || c->cfg.virtual_rank_photons > 0) { c->last_error = "shared clock and virtual ranks exclude each other"; return MCRAT_HIP_EINVAL; }
    if (c->frame_open && c->h_state && !c->h_state->done) return MCRAT_HIP_ESTATE;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->d_sc) HIPCHK(c, hipMalloc((void **)&c->d_sc, sizeof(ScState)));
    if (c->sc_own_send && c->sc_send) { (void)hipFree(c->sc_send); c->sc_send = nullptr; }
    if (c->sc_own_recv && c->sc_recv) { (void)hipFree(c->sc_recv); c->sc_recv = nullptr; }
    c->sc_own_send = c->sc_own_recv = false;
    if (c->sc_flags) { (void)hipFree(c->sc_flags); c->sc_flags = nullptr; }
    if (c->sc_gather) { (void)hipFree(c->sc_gather); c->sc_gather = nullptr; }
    c->sc_device = c->sc_peers_set = false;
    if (send) c->sc_send = (ScProposal *)send;
    else { HIPCHK(c, hipMalloc((void **)&c->sc_send, sizeof(ScProposal))); c->sc_own_send = true; }
    if (recv) c->sc_recv = (ScProposal *)recv;
    else if (world == 1) c->sc_recv = c->sc_send;
    else { HIPCHK(c, hipMalloc((void **)&c->sc_recv, sizeof(ScProposal) * world)); c->sc_own_recv = true; }
    HIPCHK(c, hipMemset(c->sc_send, 0, sizeof(ScProposal)));
    if (c->sc_recv != c->sc_send) HIPCHK(c, hipMemset(c->sc_recv, 0, sizeof(ScProposal) * world));
    c->sc_world = world;
    c->sc_rank = rank;
    c->key.slot_base = (uint32_t)slot_base;
    c->frame_open = false;
    drop_graph(c);
    return MCRAT_HIP_OK;
}

// the same attachment with the exchange done by the GPUs themselves: no host collective between propose and resolve
extern "C" int mcrat_hip_shared_clock_attach_device(mcrat_hip_ctx *c, int world, int rank, long long slot_base)
{
    int rc = mcrat_hip_shared_clock_attach(c, world, rank, slot_base, nullptr, nullptr);
    if (rc) return rc;
    if (c->sc_own_recv && c->sc_recv) (void)hipFree(c->sc_recv);
    c->sc_recv = nullptr; c->sc_own_recv = false;
    const size_t recv_bytes = sizeof(ScProposal) * 2 * (size_t)world, flag_bytes = sizeof(unsigned long long) * SC_FLAG_WORDS;
    HIPCHK(c, hipMalloc((void **)&c->sc_gather, sizeof(ScProposal) * (size_t)world));
    HIPCHK(c, hipMemset(c->sc_gather, 0, sizeof(ScProposal) * (size_t)world));
    HIPCHK(c, hipExtMallocWithFlags((void **)&c->sc_recv, recv_bytes, hipDeviceMallocFinegrained));
    c->sc_own_recv = true;
    HIPCHK(c, hipExtMallocWithFlags((void **)&c->sc_flags, flag_bytes, hipDeviceMallocFinegrained));
    HIPCHK(c, hipMemset(c->sc_recv, 0, recv_bytes));
    HIPCHK(c, hipMemset(c->sc_flags, 0, flag_bytes));
    HIPCHK(c, hipDeviceSynchronize());
    c->sc_device = true;
    c->sc_fold = true;
    if (const char *e = getenv("MCRAT_HIP_SC_FOLD")) c->sc_fold = atoi(e) != 0;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_peer_buffers(mcrat_hip_ctx *c, void **recv, size_t *recv_bytes, void **flags, size_t *flags_bytes)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->sc_device) return MCRAT_HIP_ESTATE;
    if (recv) *recv = c->sc_recv;
    if (recv_bytes) *recv_bytes = sizeof(ScProposal) * 2 * (size_t)c->sc_world;
    if (flags) *flags = c->sc_flags;
    if (flags_bytes) *flags_bytes = sizeof(unsigned long long) * SC_FLAG_WORDS;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_set_peers(mcrat_hip_ctx *c, void *const *peer_recv, void *const *peer_flags)
{
    if (!c || !peer_recv || !peer_flags) return MCRAT_HIP_EINVAL;
    if (!c->sc_device) return MCRAT_HIP_ESTATE;
    for (int r = 0; r < c->sc_world; ++r) {
        void *pr = r == c->sc_rank ? (void *)c->sc_recv : peer_recv[r], *pf = r == c->sc_rank ? (void *)c->sc_flags : peer_flags[r];
        if (!pr || !pf) return MCRAT_HIP_EINVAL;
        c->sc_peers.recv[r] = static_cast<ScProposal *>(pr);
        c->sc_peers.flag[r] = static_cast<unsigned long long *>(pf);
    }
    c->sc_peers_set = true;
    return MCRAT_HIP_OK;
}

static int sc_wait_spins()
{
    int spins = 4000000;                                             // a few seconds: ranks enter a frame together (a barrier on the host)
    if (const char *e = getenv("MCRAT_HIP_SC_WAIT_SPINS")) spins = atoi(e) > 0 ? atoi(e) : spins;
    return spins;
}

// the exchange inside the round's own kernels (launch.hpp, ScFold), when the GPUs do it themselves
static ScFold sc_fold_of(const mcrat_hip_ctx *c)
{
    ScFold f{};
    f.on = (c->sc_device && c->sc_peers_set && c->sc_fold) ? 1 : 0;
    if (f.on) {
        f.world = c->sc_world; f.rank = c->sc_rank; f.max_spins = sc_wait_spins();
        f.peers = c->sc_peers; f.my_flags = c->sc_flags; f.recv = c->sc_recv; f.gathered = c->sc_gather;
    }
    return f;
}

extern "C" int mcrat_hip_shared_clock_exchange_push(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->sc_device || !c->sc_peers_set || !c->frame_open) return MCRAT_HIP_ESTATE;
    if (c->sc_fold) return MCRAT_HIP_OK;                              // (the propose kernel has pushed)
    HIPCHK(c, launch_sc_push(c->sc_send, c->sc_peers, c->sc_flags, c->sc_world, c->sc_rank, c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_exchange_wait(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->sc_device || !c->sc_peers_set || !c->frame_open) return MCRAT_HIP_ESTATE;
    if (c->sc_fold) return MCRAT_HIP_OK;                              // (the resolve kernel will wait)
    HIPCHK(c, launch_sc_wait(c->sc_flags, c->sc_recv, c->sc_gather, c->sc_world, sc_wait_spins(), c->d_state, c->stream));
    return MCRAT_HIP_OK;
}

// After a wait has given up (mcrat_hip_shared_clock_poll answers MCRAT_HIP_EHIP) the ranks' round numbers may be out of step.  Every rank calls this --
// its give-up word, its round number and the stamps its peers left are cleared --, then the ranks synchronise (any barrier: a peer must not push
// its first new round before this rank has cleared its stamps), then begin_frame as usual.
extern "C" int mcrat_hip_shared_clock_reset_exchange(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (!c->sc_device) return MCRAT_HIP_ESTATE;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(c->sc_flags, 0, sizeof(unsigned long long) * (size_t)SC_FLAG_WORDS));
    c->frame_open = false;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_exchange(mcrat_hip_ctx *c)
{
    int rc = mcrat_hip_shared_clock_exchange_push(c);
    return rc ? rc : mcrat_hip_shared_clock_exchange_wait(c);
}

extern "C" int mcrat_hip_shared_clock_buffers(mcrat_hip_ctx *c, void **send, void **recv)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->sc_world <= 0) return MCRAT_HIP_ESTATE;
    if (send) *send = c->sc_send;
    if (recv) *recv = c->sc_recv;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_propose(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->sc_world <= 0 || !c->frame_open) return MCRAT_HIP_ESTATE;
    if (c->sc_device && !c->sc_peers_set && c->sc_fold) { c->last_error = "shared clock: the peers' buffers are not set (mcrat_hip_shared_clock_set_peers)"; return MCRAT_HIP_ESTATE; }
    HIPCHK(c, launch_sc_propose(c->kc, c->find_switch != 0, c->ph, c->hy, c->d_state, c->d_sc, c->key, c->partials, c->step_blocks,
                                c->shortlist, c->sc_send, sc_fold_of(c), c->stream));
    c->find_switch = 0;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_resolve(mcrat_hip_ctx *c)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->sc_world <= 0 || !c->frame_open) return MCRAT_HIP_ESTATE;
    const ScProposal *all = c->sc_device ? c->sc_gather : c->sc_recv;                   // device exchange: the wait kernel has copied the round out
    HIPCHK(c, launch_sc_resolve(c->kc, c->ph, c->hy, c->d_state, c->d_sc, c->key, all, c->sc_world, sc_fold_of(c), c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_poll(mcrat_hip_ctx *c, int *frame_done, mcrat_hip_frame_stats *stats)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->sc_world <= 0 || !c->frame_open) return MCRAT_HIP_ESTATE;
    HIPCHK(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(LoopState), hipMemcpyDeviceToHost, c->stream));
    unsigned long long gave_up = 0;
    if (c->sc_device) HIPCHK(c, hipMemcpyAsync(&gave_up, c->sc_flags + SC_GAVE_UP_WORD, sizeof gave_up, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (gave_up) { c->last_error = "shared clock: a peer's proposal did not arrive (device-initiated exchange gave up waiting)"; return MCRAT_HIP_EHIP; }
    if (frame_done) *frame_done = c->h_state->done == LOOP_DONE;
    fill_stats(c, stats);
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_shared_clock_finish(mcrat_hip_ctx *c, mcrat_hip_frame_stats *stats)
{
    if (!c) return MCRAT_HIP_EINVAL;
    if (c->sc_world <= 0 || !c->frame_open) return MCRAT_HIP_ESTATE;
    int rc;
    if ((rc = flush_pending(c))) return rc;
    return mcrat_hip_shared_clock_poll(c, nullptr, stats);
}

// ---------------------------------------------------------------------------------------------- reductions
static int run_reduce(mcrat_hip_ctx *c, ReducePartial &t)
{
    if (!c->have_photons) return MCRAT_HIP_ESTATE;
    int rc = flush_pending(c);
    if (rc) return rc;
    const int blocks = std::min(mcrat_hip_ctx::RED_BLOCKS, std::max(1, (c->ph.n + 255) / 256));
    HIPCHK(c, launch_reduce(c->ph, c->d_red, blocks, c->cfg.cyclosynchrotron_switch, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_red, c->d_red, sizeof(ReducePartial) * blocks, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t = c->h_red[0];
    for (int b = 1; b < blocks; ++b) {
        const ReducePartial &p = c->h_red[b];
        t.r_min = std::min(t.r_min, p.r_min); t.r_max = std::max(t.r_max, p.r_max);
        t.th_min = std::min(t.th_min, p.th_min); t.th_max = std::max(t.th_max, p.th_max);
        t.sum_scatt += p.sum_scatt; t.sum_r += p.sum_r; t.e_sum += p.e_sum; t.w_sum += p.w_sum;
        t.max_scatt = std::max(t.max_scatt, p.max_scatt); t.min_scatt = std::min(t.min_scatt, p.min_scatt);
        t.count += p.count;
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_ph_minmax(mcrat_hip_ctx *c, double *min_r, double *max_r, double *min_theta, double *max_theta)
{
    if (!c || !min_r || !max_r || !min_theta || !max_theta) return MCRAT_HIP_EINVAL;
    ReducePartial t;
    int rc = run_reduce(c, t);
    if (rc) return rc;
    *min_r = t.r_min; *max_r = t.r_max; *min_theta = t.th_min; *max_theta = t.th_max;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_scatt_stats(mcrat_hip_ctx *c, int *max_scatt, int *min_scatt, double *avg_scatt, double *avg_r)
{
    if (!c || !max_scatt || !min_scatt || !avg_scatt || !avg_r) return MCRAT_HIP_EINVAL;
    ReducePartial t;
    int rc = run_reduce(c, t);
    if (rc) return rc;
    *max_scatt = (int)t.max_scatt; *min_scatt = (int)t.min_scatt;
    *avg_scatt = t.sum_scatt / (double)t.count; *avg_r = t.sum_r / (double)t.count;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_avg_energy(mcrat_hip_ctx *c, double *erg)
{
    if (!c || !erg) return MCRAT_HIP_EINVAL;
    ReducePartial t;
    int rc = run_reduce(c, t);
    if (rc) return rc;
    *erg = (t.e_sum * C_LIGHT) / t.w_sum;
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- the analysis products' device blocks
// Block `which` with room for `need` bytes: the pool's when c is a view.  The block may be replaced, so nothing may still read the old one: c's
// stream is drained first, and that of h -- another context whose staged frame the product reads, or nullptr -- because the frame is staged there.
static int analysis_block(mcrat_hip_ctx *c, const mcrat_hip_ctx *h, int which, size_t need, char **d)
{
    mcrat_hip_ctx *owner = c->parent ? c->parent : c;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h && h != c) HIPCHK(c, hipStreamSynchronize(h->stream));
    mcrat_hip_ctx::DeviceBlock &b = owner->analysis[which];
    int rc = ensure_device_bytes(c, &b.buf, &b.bytes, need);
    if (rc) return rc;
    *d = static_cast<char *>(b.buf);
    return MCRAT_HIP_OK;
}

// The read-back of n columns of bytes_each bytes that lie pitch_bytes apart from `base` (device) on: column k to dst[k], where the caller wants it;
// a column that is not asked for (nullptr) is not copied.  Copies on c's stream, not waited for.
static int read_columns(mcrat_hip_ctx *c, const char *base, size_t pitch_bytes, size_t bytes_each, void *const *dst, int n)
{
    for (int k = 0; k < n; ++k)
        if (dst[k]) HIPCHK(c, hipMemcpyAsync(dst[k], base + pitch_bytes * (size_t)k, bytes_each, hipMemcpyDeviceToHost, c->stream));
    return MCRAT_HIP_OK;
}

// The photons of a call on one list (analysis_plan.hpp): c is a stand-alone context or a view, and what a pass left pending is applied.
// on_a_pool: the family's text for a pool, which is not one list.  may_be_empty: a context without photons passes, with no slots (the two fields:
// their "no photons" comes behind their other checks); the observers and the sightlines refuse it here.
static int list_photons(mcrat_hip_ctx *c, double time_now, const char *on_a_pool, bool may_be_empty, PhotonSource *src)
{
    if (!c->have_photons && !may_be_empty) return MCRAT_HIP_ESTATE;
    if (c->is_pool) { c->last_error = on_a_pool; return MCRAT_HIP_ESTATE; }
    if (c->have_photons) {
        int rc = flush_pending(c);
        if (rc) return rc;
    }
    *src = list_source(c->have_photons ? c->ph.n : 0, time_now, c->parent ? c->view_rank : 0);
    return MCRAT_HIP_OK;
}

// The photons of a call on a pool: every slot -- those beyond a list's length, and those of lists never created, are not FLAG_VALID and contribute
// nothing (windows are cleared on upload, lists only grow, grown slots are type 'N'; a selected capture included: c->ph is that capture's
// columns).  no_pool: the family's text.  No flush_pending, as in mcrat_hip_pool_summaries: a list stepped one by one through its view is read
// through the view, which flushes it -- the header says so.  (The sightlines' and the two fields' pool calls add it themselves.  They, and their
// list calls, have no clocks to give -- nullptr, 0.0 -- and read n_slots alone: such a source is not one for an observer's *_run.)
static int pool_photons(mcrat_hip_ctx *c, const double *clocks, const char *no_pool, PhotonSource *src)
{
    if (!c->is_pool) { c->last_error = no_pool; return MCRAT_HIP_ESTATE; }
    *src = pool_source(c->ph.n, c->n_ranks, c->rank_stride, clocks);
    return MCRAT_HIP_OK;
}

// Whose staged frame a product of c reads -- *h: `hydro`, or c itself for nullptr -- and what analysis_plan.hpp's rule says of it.  The callers
// have their own texts for a mismatch and for no frame; FRAME_NO_TABLE has one.
static const char *const NO_HOT_TABLE = "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first";
static FrameVerdict frame_of(const mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, bool with_table, bool need_cells, const mcrat_hip_ctx **h)
{
    const mcrat_hip_ctx *f = *h = hydro ? hydro : c;
    return frame_verdict(FrameSwitches{c->kc.dimensions, c->kc.geometry, c->kc.table, c->cfg.device}, FrameSwitches{f->kc.dimensions, f->kc.geometry, f->kc.table, f->cfg.device},
                         f == c, f->have_hydro, f->hy.M, f->hy.hot_table != nullptr, with_table, need_cells);
}

// A cube job, what mcrat_hip_observe and mcrat_hip_observe_sky share (observe_plan.hpp, sky_plan.hpp): the block is the cube's seven planes, the
// per-observer counters and, behind them, `in` -- the kernel's inputs in the order it stages them, then the lists' clocks when there are any.  One
// memset, one copy of the inputs, one launch, the planes and counters read back to wherever *out wants them.  `a` comes with everything but its
// device pointers; launch(a) returns an MCRAT_HIP_* code.
template <class Plan, class Dev, class Launch, class Out>
static int cube_run(mcrat_hip_ctx *c, int which, const Plan &plan, const std::vector<double> &in, bool clocks, Dev a, Launch launch, Out *out)
{
    char *d = nullptr;
    int rc = analysis_block(c, nullptr, which, plan.out_bytes + sizeof(double) * in.size(), &d);
    if (rc) return rc;
    double *d_in = reinterpret_cast<double *>(d + plan.out_bytes);
    a.staged = d_in;
    a.clocks = clocks ? d_in + plan.staged_doubles : nullptr;
    a.cube = reinterpret_cast<double *>(d);
    a.n_accepted = reinterpret_cast<unsigned long long *>(d + plan.cube_bytes);
    a.n_outside = a.n_accepted + plan.n_obs;
    HIPCHK(c, hipMemsetAsync(d, 0, plan.out_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_in, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch(a))) return rc;
    const size_t plane = sizeof(double) * (size_t)plan.n_bins, counters = sizeof(long long) * (size_t)plan.n_obs;
    void *planes[OBSERVE_PLANES] = {out->count, out->w, out->we, out->i, out->q, out->u, out->v};
    void *per_observer[2] = {out->n_accepted, out->n_outside};
    static_assert(sizeof(long long) == 8, "the count plane and the counters are read back as they are");
    if ((rc = read_columns(c, d, plane, plane, planes, OBSERVE_PLANES)) || (rc = read_columns(c, d + plan.cube_bytes, counters, counters, per_observer, 2))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- mock observations
// The photons of c->ph that src names binned by observer, detection time and energy (observe_plan.hpp, observe.hip), and the cube read back.
static int observe_run(mcrat_hip_ctx *c, const mcrat_hip_observer *obs, const PhotonSource &src, mcrat_hip_observation *out)
{
    c->obs_path = OBSERVE_PATH_NONE;
    if (!obs->cos_obs || !obs->sin_obs || !obs->cos_lo || !obs->cos_hi || !obs->t_edges || !obs->e_edges) {
        c->last_error = "observe: a null array in mcrat_hip_observer";
        return MCRAT_HIP_EINVAL;
    }
    ObservePath forced;
    ObservePlan plan;
    ObserveRefusal why = observe_path_switch(getenv("MCRAT_HIP_OBSERVE_PATH"), &forced);
    if (why == OBSERVE_OK) why = observe_plan(obs->n_obs, obs->cos_lo, obs->cos_hi, obs->n_t, obs->t_edges, obs->n_e, obs->e_edges, forced, &plan);
    if (why != OBSERVE_OK) { c->last_error = observe_refusal_text(why); return MCRAT_HIP_EINVAL; }

    // the inputs in the order the kernel stages them, the clocks behind them
    const size_t n_obs = (size_t)plan.n_obs;
    std::vector<double> in;
    in.reserve(plan.staged_doubles + (size_t)src.n_clocks);
    for (const double *v : {obs->cos_obs, obs->sin_obs, obs->cos_lo, obs->cos_hi}) in.insert(in.end(), v, v + n_obs);
    in.insert(in.end(), obs->t_edges, obs->t_edges + plan.n_t + 1); in.insert(in.end(), obs->e_edges, obs->e_edges + plan.n_e + 1);
    if (src.clocks) in.insert(in.end(), src.clocks, src.clocks + src.n_clocks);

    ObserveDev a{};
    a.n_slots = src.n_slots; a.n_obs = plan.n_obs; a.n_t = plan.n_t; a.n_e = plan.n_e; a.n_bins = plan.n_bins;
    a.slots_per_clock = src.slots_per_clock;
    a.time_now = src.time_now;
    const int rc = cube_run(c, mcrat_hip_ctx::BLOCK_OBSERVE, plan, in, src.clocks != nullptr, a, [&](const ObserveDev &dev) -> int {
        HIPCHK(c, launch_observe(c->ph, dev, plan, c->kc.stokes != 0, device_cus(c), c->stream));
        return MCRAT_HIP_OK;
    }, out);
    if (rc) return rc;
    c->obs_path = plan.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_observe(mcrat_hip_ctx *c, const mcrat_hip_observer *obs, double time_now, mcrat_hip_observation *out)
{
    if (!c || !obs || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, time_now, "observe: a rank pool's lists have clocks of their own (mcrat_hip_pool_observe, or mcrat_hip_observe on a view)", false, &src);
    return rc ? rc : observe_run(c, obs, src, out);
}

extern "C" int mcrat_hip_pool_observe(mcrat_hip_ctx *c, const mcrat_hip_observer *obs, const double *time_now, mcrat_hip_observation *out)
{
    if (!c || !obs || !time_now || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, time_now, "pool_observe: the context is no rank pool", &src);
    return rc ? rc : observe_run(c, obs, src, out);
}

extern "C" int mcrat_hip_observe_path(const mcrat_hip_ctx *c) { return c ? c->obs_path : 0; }

// ---------------------------------------------------------------------------------------------- sky observers: any direction, with images
// The caller's struct as sky_plan.hpp's checks read it, after the pointers no check may do without.
static int sky_args(mcrat_hip_ctx *c, const mcrat_hip_sky_observer *obs, SkyArgs *args)
{
    if (!obs->n0 || !obs->n1 || !obs->n2 || !obs->cos_acc || !obs->t_edges || !obs->e_edges || (obs->n_x > 0 && !obs->x_edges) || (obs->n_y > 0 && !obs->y_edges)) {
        c->last_error = "observe_sky: a null array in mcrat_hip_sky_observer";
        return MCRAT_HIP_EINVAL;
    }
    *args = SkyArgs{obs->n_obs, obs->n0, obs->n1, obs->n2, obs->cos_acc, obs->x0, obs->x1, obs->x2, obs->y0, obs->y1, obs->y2,
                    obs->n_t, obs->t_edges, obs->n_e, obs->e_edges, obs->n_x, obs->x_edges, obs->n_y, obs->y_edges};
    return MCRAT_HIP_OK;
}

// A cube job's inputs: the observers' in the order the kernel stages them (analysis_plan.hpp), `more` further edges behind them (nullptr: none), then
// the lists' clocks when there are any.
static std::vector<double> staged_inputs(const SkyArgs &s, bool axes, bool image, size_t staged_doubles, const double *more, size_t n_more, const PhotonSource &src)
{
    std::vector<double> in;
    in.reserve(staged_doubles + (size_t)src.n_clocks);
    stage_observer_inputs(s, axes, true, image, &in);
    if (more) in.insert(in.end(), more, more + n_more);
    if (src.clocks) in.insert(in.end(), src.clocks, src.clocks + src.n_clocks);
    return in;
}

// The photons of c->ph that src names binned by observer, detection time, energy and sky-plane position (sky_plan.hpp, sky.hip), and the cube read
// back.
static int sky_run(mcrat_hip_ctx *c, const mcrat_hip_sky_observer *obs, const PhotonSource &src, mcrat_hip_sky_observation *out)
{
    c->sky_path = OBSERVE_PATH_NONE;
    SkyArgs args;
    int rc = sky_args(c, obs, &args);
    if (rc) return rc;
    SkyPlan plan;
    const SkyRefusal why = sky_plan(args, getenv("MCRAT_HIP_SKY_PATH"), &plan);
    if (why != SKY_OK) { c->last_error = sky_refusal_text(why); return MCRAT_HIP_EINVAL; }

    SkyDev a{};
    a.n_slots = src.n_slots; a.n_obs = plan.n_obs; a.n_t = plan.n_t; a.n_e = plan.n_e; a.n_x = plan.n_x; a.n_y = plan.n_y; a.n_bins = plan.n_bins;
    a.slots_per_clock = src.slots_per_clock;
    a.time_now = src.time_now;
    const std::vector<double> in = staged_inputs(args, plan.image, plan.image, plan.staged_doubles, nullptr, 0, src);
    rc = cube_run(c, mcrat_hip_ctx::BLOCK_SKY, plan, in, src.clocks != nullptr, a, [&](const SkyDev &dev) -> int {
        HIPCHK(c, launch_sky(c->ph, dev, plan, c->kc.stokes != 0, sky_grid(plan, src.n_slots, device_cus(c)), c->stream));
        return MCRAT_HIP_OK;
    }, out);
    if (rc) return rc;
    c->sky_path = plan.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_observe_sky(mcrat_hip_ctx *c, const mcrat_hip_sky_observer *obs, double time_now, mcrat_hip_sky_observation *out)
{
    if (!c || !obs || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, time_now, "observe_sky: a rank pool's lists have clocks of their own (mcrat_hip_pool_observe_sky, or mcrat_hip_observe_sky on a view)", false, &src);
    return rc ? rc : sky_run(c, obs, src, out);
}

extern "C" int mcrat_hip_pool_observe_sky(mcrat_hip_ctx *c, const mcrat_hip_sky_observer *obs, const double *time_now, mcrat_hip_sky_observation *out)
{
    if (!c || !obs || !time_now || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, time_now, "pool_observe_sky: the context is no rank pool", &src);
    return rc ? rc : sky_run(c, obs, src, out);
}

extern "C" int mcrat_hip_observe_sky_path(const mcrat_hip_ctx *c) { return c ? c->sky_path : 0; }

// ---------------------------------------------------------------------------------------------- line-of-sight optical depths
// n rays marched through a staged frame (sightline_plan.hpp, sightline.hip) and the per-ray results read back.  rays: the caller's seven host
// arrays r0, r1, r2, p0 .. p3, or nullptr -- then the rays are the n slots of c->ph.  hydro: the context whose staged frame the rays cross, or
// nullptr for c's own.
static int sightline_run(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, int n, const double *const *rays,
                         mcrat_hip_sightlines *out)
{
    const mcrat_hip_ctx *h = nullptr;
    const FrameVerdict frame = frame_of(c, hydro, true, false, &h);
    if (!h->have_hydro) { c->last_error = "sightline: no staged hydro frame"; return MCRAT_HIP_ESTATE; }       // (here the frame comes first, the arguments last)
    if (frame == FRAME_MISMATCH) {
        c->last_error = "sightline: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY, TAU_CALCULATION) or on another device";
        return MCRAT_HIP_EINVAL;
    }
    if (frame == FRAME_NO_TABLE) { c->last_error = NO_HOT_TABLE; return MCRAT_HIP_ESTATE; }
    const SightlineParams p{params->step_frac, params->h_min, params->max_steps, params->tau_stop, params->surface_level};
    int forced;
    SightlinePlan plan;
    const SightlineRefusal bad_switch = sightline_refill_switch(getenv("MCRAT_HIP_SIGHTLINE_REFILL"), &forced);
    SightlineRefusal why = sightline_plan(n, p, forced, &plan);
    if (why == SIGHTLINE_OK) why = bad_switch;                   // (what the arguments are refused for comes first)
    if (why != SIGHTLINE_OK) { c->last_error = sightline_refusal_text(why); return MCRAT_HIP_EINVAL; }

    char *d = nullptr;
    int rc = analysis_block(c, h, mcrat_hip_ctx::BLOCK_SIGHTLINE, plan.ray_offset + (rays ? plan.ray_bytes : 0), &d);
    if (rc) return rc;
    const int blocks = sightline_grid(plan, device_cus(c));
    SightlineDev a{};
    a.n = n;
    a.step_frac = p.step_frac; a.h_min = p.h_min; a.max_steps = p.max_steps; a.tau_stop = p.tau_stop; a.surface_level = p.surface_level;
    a.head = reinterpret_cast<unsigned long long *>(d);
    a.f8 = reinterpret_cast<double *>(d + plan.f8_offset);
    a.i4 = reinterpret_cast<int *>(d + plan.i4_offset);
    a.refill = plan.refill ? 1 : 0;
    a.own_rays = plan.refill ? sightline_own_rays(n, blocks) : 0;
    HIPCHK(c, hipMemsetAsync(d, 0, sizeof(unsigned long long) * SIGHTLINE_HEAD_WORDS, c->stream));
    if (rays) {
        double *d_ray = reinterpret_cast<double *>(d + plan.ray_offset);
        for (int k = 0; k < SIGHTLINE_RAY_PLANES; ++k)
            HIPCHK(c, hipMemcpyAsync(d_ray + (size_t)k * (size_t)n, rays[k], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        a.ray = d_ray;
    }
    HIPCHK(c, launch_sightline(c->kc, c->ph, h->hy, a, blocks, c->stream));
    void *f8[SIGHTLINE_F8_PLANES] = {out->tau, out->path, out->surface_r0, out->surface_r1, out->surface_r2};
    void *i4[SIGHTLINE_I4_PLANES] = {out->steps, out->status, out->surface_step};
    const size_t f8_bytes = sizeof(double) * (size_t)n, i4_bytes = sizeof(int) * (size_t)n;           // (the planes' pitch: sightline_f8_plane, sightline_i4_plane)
    if ((rc = read_columns(c, d + plan.f8_offset, f8_bytes, f8_bytes, f8, SIGHTLINE_F8_PLANES)) ||
        (rc = read_columns(c, d + plan.i4_offset, i4_bytes, i4_bytes, i4, SIGHTLINE_I4_PLANES))) return rc;
    static_assert(sizeof(long long) == 8, "the status counts are read back as they are");
    HIPCHK(c, hipMemcpyAsync(out->n_status, d, sizeof(long long) * SIGHTLINE_N_STATUS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_sightline_rays(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, int n, const double *r0,
                                        const double *r1, const double *r2, const double *p0, const double *p1, const double *p2, const double *p3,
                                        mcrat_hip_sightlines *out)
{
    if (!c || !params || !out) return MCRAT_HIP_EINVAL;
    if (n > 0 && (!r0 || !r1 || !r2 || !p0 || !p1 || !p2 || !p3)) { c->last_error = "sightline: a null ray array"; return MCRAT_HIP_EINVAL; }
    if (c->have_photons) {
        int rc = flush_pending(c);
        if (rc) return rc;
    }
    const double *const rays[SIGHTLINE_RAY_PLANES] = {r0, r1, r2, p0, p1, p2, p3};
    return sightline_run(c, hydro, params, n, rays, out);
}

extern "C" int mcrat_hip_sightline_photons(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, mcrat_hip_sightlines *out)
{
    if (!c || !params || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, 0.0, "sightline: one list is a stand-alone context or a view of a pool (mcrat_hip_pool_sightline_photons takes the pool)", false, &src);
    return rc ? rc : sightline_run(c, hydro, params, src.n_slots, nullptr, out);
}

extern "C" int mcrat_hip_pool_sightline_photons(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, mcrat_hip_sightlines *out)
{
    if (!c || !params || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;                            // (the rays have no clocks)
    int rc = pool_photons(c, nullptr, "pool_sightline_photons: the context is no rank pool", &src);
    if (!rc) rc = flush_pending(c);              // (unlike the observers' pool calls)
    return rc ? rc : sightline_run(c, hydro, params, src.n_slots, nullptr, out);
}

// ---------------------------------------------------------------------------------------------- escape-weighted sky observations
// The checks of escape_plan.hpp on the caller's struct, then the frame: *h is the context whose staged frame the accepted photons are marched
// through.  EINVAL comes before ESTATE, in the order the header gives.
static int escape_check(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_escape_observer *obs, EscapeArgs *args, EscapePlan *plan,
                        const mcrat_hip_ctx **h_out)
{
    char text[ESCAPE_TEXT_BYTES];
    if (sky_args(c, &obs->sky, &args->sky) || !obs->tau_edges) {
        c->last_error = "observe_escaping: a null array in mcrat_hip_escape_observer";
        return MCRAT_HIP_EINVAL;
    }
    args->n_tau = obs->n_tau; args->tau_edges = obs->tau_edges;
    args->march = SightlineParams{obs->march.step_frac, obs->march.h_min, obs->march.max_steps, obs->march.tau_stop, -1.0};
    const EscapeRefusal why = escape_plan(*args, getenv("MCRAT_HIP_ESCAPE_PATH"), plan);
    if (why != ESCAPE_OK) { c->last_error = escape_refusal_text(why, text); return MCRAT_HIP_EINVAL; }
    switch (frame_of(c, hydro, true, false, h_out)) {
    case FRAME_MISMATCH: c->last_error = escape_refusal_text(ESCAPE_HYDRO_MISMATCH, text); return MCRAT_HIP_EINVAL;
    case FRAME_NONE: c->last_error = "observe_escaping: no staged hydro frame"; return MCRAT_HIP_ESTATE;
    case FRAME_NO_TABLE: c->last_error = NO_HOT_TABLE; return MCRAT_HIP_ESTATE;
    case FRAME_OK: break;
    }
    return MCRAT_HIP_OK;
}

// How the block's results come back.  A small block -- light curves, spectra -- is read back whole by one copy and handed out on the host: fourteen
// copies of a few hundred bytes each cost the light-curve call 0.12 ms of its 0.50.  A larger one -- images, megabytes per
// plane -- is read plane by plane, as cube_run does: a plane the caller does not ask for is not copied.
constexpr size_t ESCAPE_ONE_COPY_BYTES = 256 * 1024;

// -> planes, per-observer counters and the call's counters from `block`, host memory that holds the first out_bytes of the device block from
// `first` on (first == 0: all of it; first == plan.head_offset: the head alone), to wherever *out wants them
static void escape_fill_outputs(const EscapePlan &plan, const char *block, size_t first, mcrat_hip_escape_observation *out)
{
    static_assert(sizeof(long long) == 8, "the count plane, the counters and the head are handed over as they are");
    if (first == 0) {
        const size_t plane = sizeof(double) * (size_t)plan.n_bins, counters = sizeof(long long) * (size_t)plan.n_obs;
        void *planes[ESCAPE_PLANES] = {out->count, out->w, out->we, out->i, out->q, out->u, out->v, out->wx, out->wex};
        for (int k = 0; k < ESCAPE_PLANES; ++k)
            if (planes[k]) memcpy(planes[k], block + plane * (size_t)k, plane);
        long long *per_observer[ESCAPE_COUNTERS] = {out->n_accepted, out->n_outside, out->n_opaque, out->n_unresolved};
        for (int k = 0; k < ESCAPE_COUNTERS; ++k)
            if (per_observer[k]) memcpy(per_observer[k], block + plan.counters_offset + counters * (size_t)k, counters);
    }
    long long head[ESCAPE_HEAD_WORDS];
    memcpy(head, block + (plan.head_offset - first), sizeof head);
    for (int k = 0; k < SIGHTLINE_N_STATUS; ++k) out->n_status[k] = head[k];
    out->n_selected = head[ESCAPE_SELECTED_WORD];
    out->n_observable = head[ESCAPE_OBSERVABLE_WORD];
}

// The photons of c->ph that src names and an observer accepts, marched through h's staged frame and binned (escape_plan.hpp, escape.hip): check,
// block, stage -- the sky observation's inputs, then tau_edges, the clocks behind them --, three launches, the read-back (escape_fill_outputs), one
// synchronise, the outputs filled in.
static int escape_run(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_escape_observer *obs, const PhotonSource &src, mcrat_hip_escape_observation *out)
{
    c->esc_path = OBSERVE_PATH_NONE;
    EscapeArgs args{};
    EscapePlan plan;
    const mcrat_hip_ctx *h = nullptr;
    int rc = escape_check(c, hydro, obs, &args, &plan, &h);
    if (rc) return rc;

    const int n_slots = src.n_slots;
    const EscapeLayout lay = escape_layout(plan, n_slots, src.clocks ? src.n_clocks : 0);
    char *d = nullptr;
    if ((rc = analysis_block(c, h, mcrat_hip_ctx::BLOCK_ESCAPE, lay.total_bytes, &d))) return rc;

    const std::vector<double> in = staged_inputs(args.sky, plan.image, plan.image, plan.staged_doubles, args.tau_edges, (size_t)plan.n_tau + 1, src);
    HIPCHK(c, hipMemsetAsync(d, 0, plan.out_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + lay.staged_offset, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, c->stream));

    EscapeDev a{};
    a.n_slots = n_slots; a.n_obs = plan.n_obs; a.n_tau = plan.n_tau; a.n_t = plan.n_t; a.n_e = plan.n_e; a.n_x = plan.n_x; a.n_y = plan.n_y; a.n_bins = plan.n_bins;
    a.step_frac = plan.march.step_frac; a.h_min = plan.march.h_min; a.max_steps = plan.march.max_steps; a.tau_stop = plan.march.tau_stop;
    a.staged = reinterpret_cast<const double *>(d + lay.staged_offset);
    a.clocks = src.clocks ? reinterpret_cast<const double *>(d + lay.clocks_offset) : nullptr;
    a.slots_per_clock = src.slots_per_clock;
    a.time_now = src.time_now;
    a.cube = reinterpret_cast<double *>(d);
    a.counters = reinterpret_cast<unsigned long long *>(d + plan.counters_offset);
    a.head = reinterpret_cast<unsigned long long *>(d + plan.head_offset);
    a.tau = reinterpret_cast<double *>(d + lay.tau_offset);
    a.index = reinterpret_cast<int *>(d + lay.index_offset);
    a.status = reinterpret_cast<int *>(d + lay.status_offset);
    const int cus = device_cus(c);
    HIPCHK(c, launch_escape(c->kc, c->ph, h->hy, a, plan, c->kc.stokes != 0, escape_select_grid(n_slots, cus), escape_march_grid(n_slots),
                            escape_bin_grid(plan, n_slots, cus), c->stream));

    const bool whole = plan.out_bytes <= ESCAPE_ONE_COPY_BYTES;
    const size_t first = whole ? 0 : plan.head_offset;
    std::vector<char> host(plan.out_bytes - first);
    if (!whole) {                                // the planes and per-observer counters that *out asks for, each straight to where it wants them
        const size_t plane = sizeof(double) * (size_t)plan.n_bins, counters = sizeof(long long) * (size_t)plan.n_obs;
        void *planes[ESCAPE_PLANES] = {out->count, out->w, out->we, out->i, out->q, out->u, out->v, out->wx, out->wex};
        void *per_observer[ESCAPE_COUNTERS] = {out->n_accepted, out->n_outside, out->n_opaque, out->n_unresolved};
        if ((rc = read_columns(c, d, plane, plane, planes, ESCAPE_PLANES)) ||
            (rc = read_columns(c, d + plan.counters_offset, counters, counters, per_observer, ESCAPE_COUNTERS))) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(host.data(), d + first, host.size(), hipMemcpyDeviceToHost, c->stream));          // all of it, or the head, which lies last
    HIPCHK(c, hipStreamSynchronize(c->stream));
    escape_fill_outputs(plan, host.data(), first, out);
    c->esc_path = plan.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_observe_escaping(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_escape_observer *obs, double time_now,
                                          mcrat_hip_escape_observation *out)
{
    if (!c || !obs || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, time_now, "observe_escaping: a rank pool's lists have clocks of their own (mcrat_hip_pool_observe_escaping, or mcrat_hip_observe_escaping on a view)", false, &src);
    return rc ? rc : escape_run(c, hydro, obs, src, out);
}

extern "C" int mcrat_hip_pool_observe_escaping(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_escape_observer *obs, const double *time_now,
                                               mcrat_hip_escape_observation *out)
{
    if (!c || !obs || !time_now || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, time_now, "pool_observe_escaping: the context is no rank pool", &src);
    return rc ? rc : escape_run(c, hydro, obs, src, out);
}

extern "C" int mcrat_hip_observe_escaping_path(const mcrat_hip_ctx *c) { return c ? c->esc_path : 0; }

// ---------------------------------------------------------------------------------------------- sky observations with a resampling axis
// The photons of c->ph that src names binned as sky_run bins them, with a replica axis behind the observer and, on request, Q and U in the
// observer's frame (resample_plan.hpp, resample.hip): a cube job like sky_run's, with a third per-observer counter read back beside the two.
static int resample_run(mcrat_hip_ctx *c, const mcrat_hip_resample_observer *obs, const PhotonSource &src, mcrat_hip_resample_observation *out)
{
    c->rs_path = RESAMPLE_PATH_NONE;
    ResampleArgs args{};
    if (sky_args(c, &obs->sky, &args.sky)) {
        c->last_error = "observe_sky_resampled: a null array in mcrat_hip_resample_observer";
        return MCRAT_HIP_EINVAL;
    }
    args.mode = obs->mode; args.n_rep = obs->n_rep; args.stokes_frame = obs->stokes_frame;
    ResamplePlan plan;
    const ResampleRefusal why = resample_plan(args, getenv("MCRAT_HIP_RESAMPLE_PATH"), &plan);
    if (why != RESAMPLE_OK) {
        char text[RESAMPLE_TEXT_BYTES];
        c->last_error = resample_refusal_text(why, text);
        return MCRAT_HIP_EINVAL;
    }
    const std::vector<double> in = staged_inputs(args.sky, plan.axes, plan.image, plan.staged_doubles, nullptr, 0, src);     // (ex and ey for SKY_PLANE too)
    const ResampleGrid grid = resample_grid(plan, src.n_slots, device_cus(c));
    ResampleDev a{};
    a.n_slots = src.n_slots; a.n_obs = plan.n_obs; a.n_rep = plan.n_rep; a.n_t = plan.n_t; a.n_e = plan.n_e; a.n_x = plan.n_x; a.n_y = plan.n_y;
    a.n_bins = plan.n_bins; a.per_rep = plan.per_rep; a.mode = plan.mode; a.axes = plan.axes ? 1 : 0;
    a.slice_reps = plan.slice_reps; a.n_slices = plan.n_slices; a.grid_x = grid.x; a.grid_y = grid.y;
    a.seed = obs->seed; a.rank_base = src.rank_base; a.rank_stride = src.rank_stride;
    a.slots_per_clock = src.slots_per_clock;
    a.time_now = src.time_now;
    const int rc = cube_run(c, mcrat_hip_ctx::BLOCK_RESAMPLE, plan, in, src.clocks != nullptr, a, [&](const ResampleDev &placed) -> int {
        ResampleDev dev = placed;
        dev.n_undefined = dev.n_outside + plan.n_obs;                  // the third counter, inside what cube_run has zeroed (plan.out_bytes)
        HIPCHK(c, launch_resample(c->ph, dev, plan, c->kc.stokes != 0, grid.x, grid.y, c->stream));
        if (out->n_frame_undefined)
            HIPCHK(c, hipMemcpyAsync(out->n_frame_undefined, dev.n_undefined, sizeof(long long) * (size_t)plan.n_obs, hipMemcpyDeviceToHost, c->stream));
        return MCRAT_HIP_OK;
    }, out);
    if (rc) return rc;
    c->rs_path = plan.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_observe_sky_resampled(mcrat_hip_ctx *c, const mcrat_hip_resample_observer *obs, double time_now, mcrat_hip_resample_observation *out)
{
    if (!c || !obs || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, time_now, "observe_sky_resampled: a rank pool's lists have clocks of their own (mcrat_hip_pool_observe_sky_resampled, or mcrat_hip_observe_sky_resampled on a view)", false, &src);
    return rc ? rc : resample_run(c, obs, src, out);
}

extern "C" int mcrat_hip_pool_observe_sky_resampled(mcrat_hip_ctx *c, const mcrat_hip_resample_observer *obs, const double *time_now, mcrat_hip_resample_observation *out)
{
    if (!c || !obs || !time_now || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, time_now, "pool_observe_sky_resampled: the context is no rank pool", &src);
    return rc ? rc : resample_run(c, obs, src, out);
}

extern "C" int mcrat_hip_observe_sky_resampled_path(const mcrat_hip_ctx *c) { return c ? c->rs_path : 0; }

// ---------------------------------------------------------------------------------------------- detected-photon event lists
// The photons of c->ph that src names as rows per observer (events_plan.hpp, events.hip): check, block, stage, the launches, the read-back, one
// synchronise, the counters handed over.
static int events_run(mcrat_hip_ctx *c, const mcrat_hip_events_observer *obs, const PhotonSource &src, mcrat_hip_events *out)
{
    const int n_slots = src.n_slots;
    if (!obs->n0 || !obs->n1 || !obs->n2 || !obs->cos_acc) {
        c->last_error = "observe_events: a null array in mcrat_hip_events_observer";
        return MCRAT_HIP_EINVAL;
    }
    const EventsArgs args{obs->n_obs, obs->n0, obs->n1, obs->n2, obs->cos_acc, obs->x0, obs->x1, obs->x2, obs->y0, obs->y1, obs->y2,
                          obs->t_lo, obs->t_hi, obs->e_lo, obs->e_hi, obs->order, obs->stokes_frame, obs->capacity, out->X != nullptr || out->Y != nullptr};
    EventsPlan plan;
    const EventsRefusal why = events_plan(args, &plan);
    if (why != EVENTS_OK) {
        char text[EVENTS_TEXT_BYTES];
        c->last_error = events_refusal_text(why, text);
        return MCRAT_HIP_EINVAL;
    }
    const EventsLayout lay = events_layout(plan, n_slots, src.clocks ? src.n_clocks : 0);
    char *d = nullptr;
    int rc = analysis_block(c, nullptr, mcrat_hip_ctx::BLOCK_EVENTS, lay.total_bytes, &d);
    if (rc) return rc;

    // the observers' vectors in the order the kernels read them, no edges; the clocks in their own part of the block
    const size_t n_obs = (size_t)plan.n_obs;
    const SkyArgs vectors{plan.n_obs, args.n0, args.n1, args.n2, args.cos_acc, args.x0, args.x1, args.x2, args.y0, args.y1, args.y2};
    std::vector<double> in;
    in.reserve(plan.staged_doubles);
    stage_observer_inputs(vectors, plan.axes, false, false, &in);
    HIPCHK(c, hipMemsetAsync(d, 0, 8 * plan.head_words, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + lay.staged_offset, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, c->stream));
    if (src.clocks) HIPCHK(c, hipMemcpyAsync(d + lay.clocks_offset, src.clocks, sizeof(double) * (size_t)src.n_clocks, hipMemcpyHostToDevice, c->stream));

    EventsDev a{};
    a.n_slots = n_slots; a.n_obs = plan.n_obs; a.n_chunks = events_n_chunks(n_slots); a.chunk_slots = events_chunk_slots(n_slots);
    a.order = plan.order; a.sky_plane = plan.frame == STOKES_SKY_PLANE ? 1 : 0; a.axes = plan.axes ? 1 : 0;
    a.capacity = plan.capacity; a.n_tiles = plan.order == EVENTS_BY_TIME ? events_sort_tiles(plan.capacity) : 0;
    a.t_lo = args.t_lo; a.t_hi = args.t_hi; a.e_lo = args.e_lo; a.e_hi = args.e_hi;
    a.rank_base = src.rank_base; a.rank_stride = src.rank_stride;
    a.staged = reinterpret_cast<const double *>(d + lay.staged_offset);
    a.clocks = src.clocks ? reinterpret_cast<const double *>(d + lay.clocks_offset) : nullptr;
    a.slots_per_clock = src.slots_per_clock;
    a.time_now = src.time_now;
    unsigned long long *head = reinterpret_cast<unsigned long long *>(d);
    a.n_accepted = head; a.n_outside = head + n_obs; a.n_undefined = head + 2 * n_obs;
    a.offsets = head + events_head_offsets_word(plan);
    a.key_or = head + events_head_or_word(plan); a.key_nand = a.key_or + 1;
    a.table = reinterpret_cast<unsigned long long *>(d + lay.table_offset);
    a.rank = reinterpret_cast<int *>(d + lay.rank_offset); a.slot = reinterpret_cast<int *>(d + lay.slot_offset);
    double **f8[EVENTS_F8_COLUMNS] = {&a.t, &a.e, &a.w, &a.s0, &a.s1, &a.s2, &a.s3, &a.num_scatt, &a.X, &a.Y};
    for (int k = 0; k < (plan.axes ? EVENTS_F8_COLUMNS : EVENTS_F8_COLUMNS - 2); ++k) *f8[k] = reinterpret_cast<double *>(d + lay.f8_offset + lay.f8_pitch * (size_t)k);
    a.type = d + lay.type_offset;
    if (plan.order == EVENTS_BY_TIME) {
        a.sort_table = reinterpret_cast<unsigned *>(d + lay.sort_table_offset);
        a.source = reinterpret_cast<unsigned *>(d + lay.source_offset);
        for (int b = 0; b < 2; ++b) {
            a.keys[b] = reinterpret_cast<unsigned long long *>(d + lay.keys_offset + lay.keys_pitch * (size_t)b);
            a.index[b] = reinterpret_cast<unsigned *>(d + lay.index_offset + lay.index_pitch * (size_t)b);
        }
    }
    HIPCHK(c, launch_events(c->ph, a, plan, c->kc.stokes != 0, c->stream));

    // the head in one copy; every column that is asked for in full (what lies behind n_total is unspecified)
    std::vector<unsigned long long> host(plan.head_words);
    HIPCHK(c, hipMemcpyAsync(host.data(), d, 8 * plan.head_words, hipMemcpyDeviceToHost, c->stream));
    const size_t cap = (size_t)plan.capacity;
    if (cap) {
        if (out->rank) HIPCHK(c, hipMemcpyAsync(out->rank, a.rank, sizeof(int) * cap, hipMemcpyDeviceToHost, c->stream));
        if (out->slot) HIPCHK(c, hipMemcpyAsync(out->slot, a.slot, sizeof(int) * cap, hipMemcpyDeviceToHost, c->stream));
        void *wanted[EVENTS_F8_COLUMNS] = {out->t, out->e, out->w, out->s0, out->s1, out->s2, out->s3, out->num_scatt, out->X, out->Y};
        if ((rc = read_columns(c, d + lay.f8_offset, lay.f8_pitch, sizeof(double) * cap, wanted, plan.axes ? EVENTS_F8_COLUMNS : EVENTS_F8_COLUMNS - 2))) return rc;
        if (out->type) HIPCHK(c, hipMemcpyAsync(out->type, a.type, cap, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));

    static_assert(sizeof(long long) == 8, "the counters and offsets are handed over as they are");
    const unsigned long long *offsets = host.data() + events_head_offsets_word(plan);
    long long *per_observer[EVENTS_COUNTERS] = {out->n_accepted, out->n_outside, out->n_frame_undefined};
    for (int k = 0; k < EVENTS_COUNTERS; ++k)
        if (per_observer[k]) memcpy(per_observer[k], host.data() + n_obs * (size_t)k, 8 * n_obs);
    if (out->offsets) memcpy(out->offsets, offsets, 8 * (n_obs + 1));
    if (out->n_events)
        for (size_t o = 0; o < n_obs; ++o) out->n_events[o] = (long long)(offsets[o + 1] - offsets[o]);
    out->n_total = (long long)offsets[n_obs];
    out->key_or = host[events_head_or_word(plan)];
    out->key_and = ~host[events_head_or_word(plan) + 1];
    out->sort_passes_run = out->sort_passes_skipped = 0;
    const bool fits = out->n_total <= (long long)plan.capacity;
    if (plan.order == EVENTS_BY_TIME && out->n_total > 0 && fits) {
        EventsPass launched[EVENTS_MAX_PASSES], run[EVENTS_MAX_PASSES];
        const int n_launched = events_launch_list(plan.n_obs, launched);
        out->sort_passes_run = events_pass_list(out->key_or, out->key_and, plan.n_obs, run);
        out->sort_passes_skipped = n_launched - out->sort_passes_run;
    }
    const bool counting = plan.capacity == 0 && !out->rank && !out->slot && !out->t && !out->e && !out->w && !out->s0 && !out->s1 && !out->s2 && !out->s3 &&
                          !out->X && !out->Y && !out->num_scatt && !out->type;
    if (!fits && !counting) {
        char text[EVENTS_TEXT_BYTES];
        snprintf(text, sizeof text, "observe_events: the list has %lld rows, capacity is %d: no row is to be trusted (the counters are exact)", out->n_total, plan.capacity);
        c->last_error = text;
        return MCRAT_HIP_EREFUSED;
    }
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_observe_events(mcrat_hip_ctx *c, const mcrat_hip_events_observer *obs, double time_now, mcrat_hip_events *out)
{
    if (!c || !obs || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = list_photons(c, time_now, "observe_events: a rank pool's lists have clocks of their own (mcrat_hip_pool_observe_events, or mcrat_hip_observe_events on a view)", false, &src);
    return rc ? rc : events_run(c, obs, src, out);
}

extern "C" int mcrat_hip_pool_observe_events(mcrat_hip_ctx *c, const mcrat_hip_events_observer *obs, const double *time_now, mcrat_hip_events *out)
{
    if (!c || !obs || !time_now || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, time_now, "pool_observe_events: the context is no rank pool", &src);
    return rc ? rc : events_run(c, obs, src, out);
}

// ---------------------------------------------------------------------------------------------- spectral fits
// Every row of (count, W) fitted to a cutoff power law or a Band function (fit_plan.hpp, fit.hip): check, block, the inputs copied, one launch, the
// output columns read back, one synchronise.  The call reads no photon and no frame: any context will do, a view uses its pool's block.
extern "C" int mcrat_hip_fit_spectra(mcrat_hip_ctx *c, const mcrat_hip_fit_args *args, mcrat_hip_fit_result *out)
{
    if (!c || !args || !out) return MCRAT_HIP_EINVAL;
    const FitArgs fa{args->model, args->n_spec, args->n_e, args->count, args->w, args->e_edges, args->log_e, args->e_piv,
                     args->alpha_lo, args->alpha_hi, args->lambda_lo, args->lambda_hi, args->beta_lo, args->beta_hi,
                     args->g_alpha, args->g_lambda, args->g_beta, args->n_rounds, args->shrink, args->min_count};
    FitPlan plan;
    const FitRefusal why = fit_plan(fa, &plan);
    if (why != FIT_OK) { c->last_error = fit_refusal_text(why); return MCRAT_HIP_EINVAL; }
    char *d = nullptr;
    int rc = analysis_block(c, nullptr, mcrat_hip_ctx::BLOCK_FIT, plan.total_bytes, &d);
    if (rc) return rc;
    const size_t cells = (size_t)plan.n_spec * (size_t)plan.n_e, rows = (size_t)plan.n_spec;
    HIPCHK(c, hipMemcpyAsync(d + plan.edges_offset, fa.e_edges, 8 * ((size_t)plan.n_e + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + plan.log_e_offset, fa.log_e, 8 * (size_t)plan.n_e, hipMemcpyHostToDevice, c->stream));
    if (cells) {
        static_assert(sizeof(long long) == 8, "the counts are uploaded as they are");
        HIPCHK(c, hipMemcpyAsync(d + plan.count_offset, fa.count, 8 * cells, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d + plan.w_offset, fa.w, 8 * cells, hipMemcpyHostToDevice, c->stream));
    }
    FitDev a{};
    a.search = plan.search; a.n_spec = plan.n_spec; a.n_e = plan.n_e;
    a.e_edges = reinterpret_cast<const double *>(d + plan.edges_offset); a.log_e = reinterpret_cast<const double *>(d + plan.log_e_offset);
    a.count = reinterpret_cast<const long long *>(d + plan.count_offset); a.w = reinterpret_cast<const double *>(d + plan.w_offset);
    double **f8[FIT_F8_COLUMNS] = {&a.alpha, &a.beta, &a.e_peak, &a.amplitude, &a.chi2};
    for (int k = 0; k < FIT_F8_COLUMNS; ++k) *f8[k] = reinterpret_cast<double *>(d + plan.f8_offset + plan.f8_pitch * (size_t)k);
    int **i4[FIT_I4_COLUMNS] = {&a.n_used, &a.dof, &a.status};
    for (int k = 0; k < FIT_I4_COLUMNS; ++k) *i4[k] = reinterpret_cast<int *>(d + plan.i4_offset + plan.i4_pitch * (size_t)k);
    HIPCHK(c, launch_fit(a, plan, c->stream));
    if (rows) {
        void *wanted[FIT_F8_COLUMNS] = {out->alpha, out->beta, out->e_peak, out->amplitude, out->chi2};
        void *wanted_i[FIT_I4_COLUMNS] = {out->n_used, out->dof, out->status};
        if ((rc = read_columns(c, d + plan.f8_offset, plan.f8_pitch, sizeof(double) * rows, wanted, FIT_F8_COLUMNS)) ||
            (rc = read_columns(c, d + plan.i4_offset, plan.i4_pitch, sizeof(int) * rows, wanted_i, FIT_I4_COLUMNS))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- the two fields on the hydro mesh
// What the radiation field and the comoving field share: the frame whose cells the photons are located in, and the job on their block.

// *h: the context whose staged frame the photons are located in.  The caller has checked its bins: EINVAL before ESTATE, as the headers order them.
static int field_frame(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const char *mismatch, const char *no_frame, const mcrat_hip_ctx **h)
{
    switch (frame_of(c, hydro, false, true, h)) {
    case FRAME_MISMATCH: c->last_error = mismatch; return MCRAT_HIP_EINVAL;
    case FRAME_NONE: c->last_error = no_frame; return MCRAT_HIP_ESTATE;
    default: return MCRAT_HIP_OK;
    }
}

// A field job, on cube_run's model: the block for `plan`, one memset, one copy of the edges when there are any, the launch -- timed with
// cfg.profile --, the planes and the head's three counters read back to wherever *out wants them.  `a` comes with everything but its device
// pointers; launch(a, where the planes lie) returns an MCRAT_HIP_* code.
template <class Plan, class Dev, class Launch, class Out>
static int field_run(mcrat_hip_ctx *c, const mcrat_hip_ctx *h, int which, const Plan &plan, const std::vector<double> &edges, Dev a, Launch launch,
                     void *const *planes, int n_planes, Out *out)
{
    char *d = nullptr;
    int rc = analysis_block(c, h, which, plan.total_bytes, &d);
    if (rc) return rc;
    a.staged = reinterpret_cast<const double *>(d + plan.staged_offset);
    a.head = reinterpret_cast<unsigned long long *>(d);
    a.acc = reinterpret_cast<double *>(d + RADFIELD_ACC_OFFSET);
    HIPCHK(c, hipMemsetAsync(d, 0, plan.zeroed_bytes, c->stream));
    if (!edges.empty()) HIPCHK(c, hipMemcpyAsync(d + plan.staged_offset, edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice, c->stream));
    c->prof_step_ms = 0; c->prof_launches = 0;                   // (cfg.profile: the kernel's own duration, mcrat_hip_profile_totals)
    if ((rc = profiled(c, 1, [&]() -> int { return launch(a, reinterpret_cast<double *>(d + plan.planes_offset)); }))) return rc;
    const size_t plane = sizeof(double) * (size_t)plan.n_bins;
    static_assert(sizeof(long long) == 8 && COMOVING_ACC_OFFSET == RADFIELD_ACC_OFFSET, "the count plane and the counters are read back as they are; one head for both fields");
    if ((rc = read_columns(c, d + plan.planes_offset, plane, plane, planes, n_planes))) return rc;
    long long head[RADFIELD_N_SCALARS];
    HIPCHK(c, hipMemcpyAsync(head, d, sizeof(head), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_observable = head[RF_N_OBSERVABLE]; out->n_unlocated = head[RF_N_UNLOCATED]; out->n_outside = head[RF_N_OUTSIDE];
    return MCRAT_HIP_OK;
}

// The _bins entry points: the product's checks alone (`prepare`), for the number of bins.
template <class Plan, class Bins, class Prepare>
static int field_bins(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const Bins *bins, int *n_bins, Prepare prepare)
{
    if (!c || !bins || !n_bins) return MCRAT_HIP_EINVAL;
    const mcrat_hip_ctx *h = nullptr;
    Plan plan;
    int rc = prepare(c, hydro, bins, &h, &plan);
    if (rc) return rc;
    *n_bins = plan.n_bins;
    return MCRAT_HIP_OK;
}

// ---------------------------------------------------------------------------------------------- the radiation field on the hydro mesh
// The checks of radfield_plan.hpp on the caller's bins, then the frame: *plan is the block for its cells.
static int radfield_prepare(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, const mcrat_hip_ctx **h, RadfieldPlan *plan)
{
    RadfieldShape shape;
    const RadfieldRefusal why = radfield_check(bins->mode, bins->n_r, bins->r_edges, bins->n_mu, bins->mu_edges, getenv("MCRAT_HIP_RADFIELD_PATH"), &shape);
    if (why != RADFIELD_OK) { c->last_error = radfield_refusal_text(why); return MCRAT_HIP_EINVAL; }
    int rc = field_frame(c, hydro, radfield_refusal_text(RADFIELD_HYDRO_MISMATCH), "radiation_field: no staged hydro frame", h);
    if (rc) return rc;
    *plan = radfield_layout(shape, (*h)->hy.M);
    return MCRAT_HIP_OK;
}

// The n_slots slots of c->ph located in the frame of `hydro` and summed per bin (radfield_plan.hpp, radfield.hip): a field job whose launch is,
// for a bin-major build, followed by the transposition.
static int radfield_run(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, int n_slots, mcrat_hip_radfield *out)
{
    c->rf_path = OBSERVE_PATH_NONE;
    const mcrat_hip_ctx *h = nullptr;
    RadfieldPlan plan;
    int rc = radfield_prepare(c, hydro, bins, &h, &plan);
    if (rc) return rc;
    if (n_slots <= 0) { c->last_error = "radiation_field: no photons"; return MCRAT_HIP_ESTATE; }

    RadfieldDev a{};
    a.n_slots = n_slots; a.n_r = plan.s.n_r; a.n_mu = plan.s.n_mu; a.n_bins = plan.n_bins;
    std::vector<double> edges;
    if (plan.s.mode == RADFIELD_SHELLS) {
        edges.insert(edges.end(), bins->r_edges, bins->r_edges + plan.s.n_r + 1);
        edges.insert(edges.end(), bins->mu_edges, bins->mu_edges + plan.s.n_mu + 1);
    }
    const int cus = device_cus(c);
    void *planes[RADFIELD_PLANES] = {out->count, out->w, out->we_lab, out->we_comv, out->w_nscatt, out->w_temp};
    rc = field_run(c, h, mcrat_hip_ctx::BLOCK_RADFIELD, plan, edges, a, [&](const RadfieldDev &dev, double *d_planes) -> int {
        HIPCHK(c, launch_radfield(c->kc, c->ph, h->hy, dev, plan, radfield_grid(plan, n_slots, cus), c->stream));
        if (plan.bin_major) HIPCHK(c, launch_radfield_transpose(dev.acc, d_planes, plan.n_bins, cus, c->stream));
        return MCRAT_HIP_OK;
    }, planes, RADFIELD_PLANES, out);
    if (rc) return rc;
    c->rf_path = plan.s.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_radiation_field_bins(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, int *n_bins)
{
    return field_bins<RadfieldPlan>(c, hydro, bins, n_bins, radfield_prepare);
}

extern "C" int mcrat_hip_radiation_field(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, mcrat_hip_radfield *out)
{
    if (!c || !bins || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;                            // (a context without photons goes on to the checks, then "no photons")
    int rc = list_photons(c, 0.0, "radiation_field: one list is a stand-alone context or a view of a pool (mcrat_hip_pool_radiation_field takes the pool)", true, &src);
    return rc ? rc : radfield_run(c, hydro, bins, src.n_slots, out);
}

extern "C" int mcrat_hip_pool_radiation_field(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, mcrat_hip_radfield *out)
{
    if (!c || !bins || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, nullptr, "pool_radiation_field: the context is no rank pool", &src);
    if (!rc) rc = flush_pending(c);              // (unlike the observers' pool calls)
    return rc ? rc : radfield_run(c, hydro, bins, src.n_slots, out);
}

extern "C" int mcrat_hip_radiation_field_path(const mcrat_hip_ctx *c) { return c ? c->rf_path : 0; }

// ---------------------------------------------------------------------------------------------- the comoving radiation field
// The checks of comoving_plan.hpp on the caller's bins, then the frame, as radfield_prepare: *plan is the block for its cells (CELLS: the product
// of the three axes is checked here, once the cells are known).
static int comoving_prepare(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, const mcrat_hip_ctx **h, ComovingPlan *plan)
{
    ComovingShape shape;
    ComovingRefusal why = comoving_check(bins->mode, bins->n_r, bins->r_edges, bins->n_mu, bins->mu_edges, bins->n_e, bins->e_edges, bins->n_a, bins->a_edges,
                                         getenv("MCRAT_HIP_COMOVING_PATH"), &shape);
    if (why != COMOVING_OK) { c->last_error = comoving_refusal_text(why); return MCRAT_HIP_EINVAL; }
    int rc = field_frame(c, hydro, comoving_refusal_text(COMOVING_HYDRO_MISMATCH), "comoving_field: no staged hydro frame", h);
    if (rc) return rc;
    if ((why = comoving_layout(shape, (*h)->hy.M, plan)) != COMOVING_OK) { c->last_error = comoving_refusal_text(why); return MCRAT_HIP_EINVAL; }
    return MCRAT_HIP_OK;
}

// The n_slots slots of c->ph located in the frame of `hydro`, boosted and summed per bin (comoving_plan.hpp, comoving.hip): a field job.
static int comoving_run(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, int n_slots, mcrat_hip_comoving *out)
{
    c->cf_path = OBSERVE_PATH_NONE;
    const mcrat_hip_ctx *h = nullptr;
    ComovingPlan plan;
    int rc = comoving_prepare(c, hydro, bins, &h, &plan);
    if (rc) return rc;
    if (n_slots <= 0) { c->last_error = "comoving_field: no photons"; return MCRAT_HIP_ESTATE; }

    ComovingDev a{};
    a.n_slots = n_slots; a.n_r = plan.s.n_r; a.n_mu = plan.s.n_mu; a.n_e = plan.s.n_e; a.n_a = plan.s.n_a; a.n_bins = plan.n_bins;
    std::vector<double> edges;
    if (plan.s.mode == COMOVING_SHELLS) {
        edges.insert(edges.end(), bins->r_edges, bins->r_edges + plan.s.n_r + 1);
        edges.insert(edges.end(), bins->mu_edges, bins->mu_edges + plan.s.n_mu + 1);
    }
    edges.insert(edges.end(), bins->e_edges, bins->e_edges + plan.s.n_e + 1);
    edges.insert(edges.end(), bins->a_edges, bins->a_edges + plan.s.n_a + 1);
    const int cus = device_cus(c);
    void *planes[COMOVING_PLANES] = {out->count, out->w, out->we, out->wea, out->weaa, out->we_lab, out->wem, out->wemm};
    rc = field_run(c, h, mcrat_hip_ctx::BLOCK_COMOVING, plan, edges, a, [&](const ComovingDev &dev, double *) -> int {
        HIPCHK(c, launch_comoving(c->kc, c->ph, h->hy, dev, plan, comoving_grid(plan, n_slots, cus), c->stream));
        return MCRAT_HIP_OK;
    }, planes, COMOVING_PLANES, out);
    if (rc) return rc;
    c->cf_path = plan.s.path;
    return MCRAT_HIP_OK;
}

extern "C" int mcrat_hip_comoving_field_bins(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, int *n_bins)
{
    return field_bins<ComovingPlan>(c, hydro, bins, n_bins, comoving_prepare);
}

extern "C" int mcrat_hip_comoving_field(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, mcrat_hip_comoving *out)
{
    if (!c || !bins || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;                            // (a context without photons goes on to the checks, then "no photons")
    int rc = list_photons(c, 0.0, "comoving_field: one list is a stand-alone context or a view of a pool (mcrat_hip_pool_comoving_field takes the pool)", true, &src);
    return rc ? rc : comoving_run(c, hydro, bins, src.n_slots, out);
}

extern "C" int mcrat_hip_pool_comoving_field(mcrat_hip_ctx *c, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, mcrat_hip_comoving *out)
{
    if (!c || !bins || !out) return MCRAT_HIP_EINVAL;
    PhotonSource src;
    int rc = pool_photons(c, nullptr, "pool_comoving_field: the context is no rank pool", &src);
    if (!rc) rc = flush_pending(c);              // (unlike the observers' pool calls)
    return rc ? rc : comoving_run(c, hydro, bins, src.n_slots, out);
}

extern "C" int mcrat_hip_comoving_field_path(const mcrat_hip_ctx *c) { return c ? c->cf_path : 0; }

extern "C" int mcrat_hip_eval_function(mcrat_hip_ctx *c, int fn, int n, const double *in, double *out, uint64_t seed)
{
    // row widths by code (include/mcrat_hip.h): 1-7 the reference-shaped functions, 8-19 the loop's own forms
    static const int in_w[MCRAT_HIP_FN_COUNT] = {0, 1, 7, 7, 13, 5, 5, 9, 1, 1, 1, 5, 9, 9, 7, 9, 2, 3, 2, 1};
    static const int out_w[MCRAT_HIP_FN_COUNT] = {0, 1, 4, 4, 4, 4, 4, 13, 1, 1, 1, 5, 4, 4, 4, 2, 4, 3, 4, 1};
    if (!c || n <= 0 || !in || !out || fn < 1 || fn >= MCRAT_HIP_FN_COUNT) return MCRAT_HIP_EINVAL;
    // A courtesy beyond the contract (one context, one thread at a time): a look-up asked for while another thread is inside
    // mcrat_hip_create_hot_cross_section on this context is refused.  That call writes a scratch buffer and the caller's array only, never the
    // context's table, so the answer would be the look-up on whatever table the context held before -- rarely what a caller in the middle of
    // making a table means.  (No last_error here: the other thread may be writing it.)
    if (fn == MCRAT_HIP_FN_THERMAL_CROSS_SECTION && __atomic_load_n(&c->hot_creating, __ATOMIC_ACQUIRE)) return MCRAT_HIP_EINVAL;
    const size_t bi = sizeof(double) * (size_t)in_w[fn] * (size_t)n, bo = sizeof(double) * (size_t)out_w[fn] * (size_t)n;
    double *d_in = nullptr, *d_out = nullptr;
    HIPCHK(c, hipMalloc((void **)&d_in, bi));
    if (hipMalloc((void **)&d_out, bo) != hipSuccess) { (void)hipFree(d_in); return MCRAT_HIP_ENOMEM; }
    hipError_t e = hipMemcpyAsync(d_in, in, bi, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_eval_function(c->kc, c->hy, fn, n, d_in, d_out, seed, c->key.stream, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, bo, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    HIPCHK(c, e);
    return MCRAT_HIP_OK;
}

extern "C" long long mcrat_hip_covered_octants(mcrat_hip_ctx *c, int *out, long long cap)
{
    if (!c || cap < 0 || (cap > 0 && !out)) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    const GridDev &g = c->hy.grid;
    if (!g.cov_back) return 0;
    const long long n = ((long long)g.dim[0] * g.dim[1] * g.dim[2]) << g.naxes;
    if (std::min(n, cap) > 0) {
        if (hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, reinterpret_cast<const int *>(g.dir) - g.cov_back, sizeof(int) * (size_t)std::min(n, cap), hipMemcpyDeviceToHost) != hipSuccess) {
            c->last_error = "covered_octants failed";
            return MCRAT_HIP_EHIP;
        }
    }
    return n;
}

extern "C" int mcrat_hip_lookup_cell(mcrat_hip_ctx *c, int n, const double *a0, const double *a1, const double *a2, int *out)
{
    if (!c || n <= 0 || !a0 || !a1 || !out) return MCRAT_HIP_EINVAL;
    if (!c->have_hydro) return MCRAT_HIP_ESTATE;
    double *d = nullptr;
    int *dout = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, sizeof(double) * 3 * (size_t)n));
    if (hipMalloc((void **)&dout, sizeof(int) * (size_t)n) != hipSuccess) { (void)hipFree(d); return MCRAT_HIP_ENOMEM; }
    int rc = MCRAT_HIP_OK;
    std::vector<double> zeros;
    if (!a2) { zeros.assign(n, 0.0); a2 = zeros.data(); }
    if (hipMemcpy(d, a0, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, a1, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + 2 * (size_t)n, a2, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        launch_lookup(c->kc, c->hy, n, d, d + n, d + 2 * (size_t)n, dout, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(out, dout, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess) {
        c->last_error = "lookup_cell failed";
        rc = MCRAT_HIP_EHIP;
    }
    (void)hipFree(d);
    (void)hipFree(dout);
    return rc;
}
