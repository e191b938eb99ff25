// launch.hpp -- host-callable launchers of the kernels in kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "frame_queue.hpp"
#include "list_plan.hpp"
#include "hydro_plan.hpp"
#include "rank_form_plan.hpp"

namespace mcrat {

struct KernelConfig {
    int dimensions;
    int geometry;
    int stokes;
    int table;      // TAU_CALCULATION == TABLE: the kernels of kernels_table.hip
};

struct ReducePartial {      // one per workgroup of the reduction kernels
    double r_min, r_max, th_min, th_max;       // phMinMax (weight != 0)
    double sum_scatt, sum_r, e_sum, w_sum;     // phScattStats / averagePhotonEnergy
    double max_scatt, min_scatt;
    long long count;
};

int step_grid_blocks(int n_pad);   // workgroups of the step kernel for this capacity

// findContainingHydroCell + calcMeanFreePath (+ the pending updatePhotonPosition) over all slots
hipError_t launch_step(const KernelConfig &kc, bool force_relocate, const PhotonDev &ph, const HydroDev &hy,
                       LoopState *st, RngKey key, Cand *block_min, int blocks, Shortlist *sl, hipStream_t stream);
// candidate selection + photonEvent + loop bookkeeping
hipError_t launch_event(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, RngKey key,
                        const Cand *block_min, int n_blocks, Shortlist *sl, hipStream_t stream);
// ... with the caller's tape of uniforms as the random source (mcrat_hip_set_rng_tape): the pass's free-path draws in slot order
// (tape_draw_kernel, after launch_step), then the event reading on from where they stopped
struct TapeDev;
hipError_t launch_tape_pass(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, RngKey key, const TapeDev &tape,
                            Cand *block_min, int n_blocks, Shortlist *sl, hipStream_t stream);
// virtual ranks: every workgroup (of RankLaunch::threads threads) runs the whole loop of one independent photon list: the slots
// [r * rank_stride, ...) -- rank_stride of them, or desc[r].len with the list's own seed and stream (rank pool); longest_list sizes the LDS copy
// hook: (device memory) what the cyclo-synchrotron hook needs -- then lists with `cs` run it inside the loop instead of parking for
// cs_replace_pool_kernel after every pass it has to look at
// The frame queue -- ONE launch takes every list through SEVERAL hydro frames -- is frame_queue.hpp: FrameQueueDev, its items and records.
// What a context knows about its device from its creation on, so that no launch has to ask again (nullptr: the launcher asks the runtime).
struct RankDeviceInfo { int device, cus; };
// One launch of the rank loop: the lists, the form they run in, and what goes with them.
struct RankLaunch {
    int n_ranks = 0, rank_stride = 0;    // the lists: [r * rank_stride, ...), as above
    int longest_list = 0;                // sizes the LDS copy of the per-pass columns; RANK_COLUMNS_GLOBAL: the columns stay in HBM/L2
    const RankDesc *desc = nullptr;
    int threads = 256;                   // per list: 64 (with the hook only), 128, 256 or 512; anything else runs 256
    bool fuse = false;                   // the build with the fused pass, where one exists (rank_form_plan.hpp, rank_build_exists); unfused where not
    bool no_lds_lists = false;           // MCRAT_HIP_NO_LDS_LISTS is set: the columns stay in HBM/L2 whatever longest_list says
    long long max_passes = 0;            // per list and launch
    struct CsFrame *cs = nullptr;        // cyclo-synchrotron lists ...
    const struct CsHookArgs *hook = nullptr;   // ... and the hook inside the loop (above)
    const FrameQueueDev *fq = nullptr;   // n_frames > 0 makes it a queue launch: persistent workgroups, at most one per open item: n_open of them for
    int n_open = 0;                      //   the items in fq->order.  A form without a queue build: hipErrorNotSupported, and nothing is launched
    const RankDeviceInfo *dev = nullptr;
};
// The launch as rank_form_plan.hpp's rule sees it: the engine asks rank_form_resolve whether a queued launch has a build before it plans one, the
// launcher asks it for the form it launches.
inline bool rank_launch_queued(const RankLaunch &rl) { return rl.fq && rl.fq->n_frames > 0; }
inline RankFormRequest rank_form_request(const KernelConfig &kc, const RankLaunch &rl, bool queued)
{
    return RankFormRequest{rl.threads, rl.fuse, rl.cs && rl.hook && rl.desc, queued, rl.longest_list, kc.stokes != 0, kc.geometry, kc.table != 0, rl.no_lds_lists};
}
// The launcher asks the runtime once per kernel: the dynamic-LDS limit it has set for a kernel and the occupancy it was told for a (kernel, LDS size)
// are remembered (rank_launch.hip, KernelNote), so a second launch of the same form makes no hipFuncSetAttribute and no occupancy query.
// rank_launch_grid: the workgroups of the launch of `kernel`, the plan's build, after the kernel has been allowed the plan's dynamic LDS; -1: the runtime
// refuses the LDS.
int rank_launch_grid(const void *kernel, const RankLaunch &rl, const RankFormPlan &plan);
hipError_t launch_rank_loop(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *states, RngKey key, const RankLaunch &rl,
                            hipStream_t stream);
// The tape build of the rank pool (mcrat_hip_pool_set_rng_tapes): every list of a pool that holds tapes goes through it, whatever choose_rank_block
// would pick -- 256 threads per list, columns in HBM/L2, no fused pass, no frame queue.  A list with a tape takes its free-path draws and its events'
// draws from it, in MCRaT's call order, as the one-list tape path does (launch_tape_pass); a list without one draws from its keyed streams exactly as
// the keyed builds do.  Its tape is entries [offset, offset + n) of `u`; `cursor` is read when the list's frame starts and written when it ends.
struct TapeList {
    long long offset;                // the list's first entry in the pool's concatenated tape buffer
    long long n;                     // its entries (0: the list keeps its keyed streams)
    long long cursor;                // the next unread entry, relative to offset
    int error;                       // != 0: the list needed more entries than its tape holds (its results are then meaningless)
    int pad;
};
hipError_t launch_rank_loop_tape(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *states, RngKey key, int n_ranks, int rank_stride,
                                 const RankDesc *desc, const double *u, TapeList *tapes, long long max_passes, hipStream_t stream);
// shared clock with a device-initiated exchange (staging.hip): recv[r] = rank r's receive buffer (2 x world proposals, by round parity),
// flag[r] = rank r's stamps (SC_MAX_WORLD words, one per sender, + a word counting waits that gave up + the rank's own round number)
struct ScPeers { ScProposal *recv[SC_MAX_WORLD]; unsigned long long *flag[SC_MAX_WORLD]; };
constexpr int SC_GAVE_UP_WORD = SC_MAX_WORLD, SC_ROUND_WORD = SC_MAX_WORLD + 1, SC_FLAG_WORDS = SC_MAX_WORLD + 2;
// the same exchange folded into the round's own kernels (on != 0): sc_propose_kernel pushes its proposal when it has written it, sc_resolve_kernel
// waits for the round's stamps before it reads `gathered` -- two launches less per round than push and wait as kernels of their own
struct ScFold { int on, world, rank, max_spins; ScPeers peers; unsigned long long *my_flags; const ScProposal *recv; ScProposal *gathered; };
hipError_t launch_sc_push(const ScProposal *send, const ScPeers &peers, unsigned long long *my_flags, int world, int rank, hipStream_t stream);
hipError_t launch_sc_wait(unsigned long long *my_flags, const ScProposal *recv, ScProposal *gathered, int world, int max_spins, LoopState *st, hipStream_t stream);
// FAST mode: every photon through the whole frame on its own clock (kernels.hip, fast_frame_kernel); the counters add up over launches
struct FastCounts { unsigned long long photon_steps, scatterings, kn_rejections, relocated, not_found, unfinished, passes; };
// desc != nullptr: the photons are the lists of a rank pool (list r in slots [r * stride, r * stride + desc[r].len), stride a multiple of 256);
// every list then has its own seed and stream (desc), its own frame time and its own counters (counts[r]); lists with len 0 or no time stand still
struct FastLists { int stride; const RankDesc *desc; const double *remaining_time; const int *windows; };   // windows: per list (nullptr: the launch's)
hipError_t launch_fast_frame(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, RngKey key, double remaining_time, int windows,
                             int max_passes, FastCounts *counts, const FastLists &lists, hipStream_t stream);
// one list over several GPUs with one clock: {step, midpass re-read, proposal of this GPU's earliest candidates} ...
hipError_t launch_sc_propose(const KernelConfig &kc, bool force_relocate, const PhotonDev &ph, const HydroDev &hy, LoopState *st,
                             ScState *sc, RngKey key, Cand *block_min, int blocks, Shortlist *sl, ScProposal *out, const ScFold &fold, hipStream_t stream);
// ... and, after the host has all-gathered the proposals into `all`, the replicated walk of photonEvent
hipError_t launch_sc_resolve(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, ScState *sc, RngKey key,
                             const ScProposal *all, int world, const ScFold &fold, hipStream_t stream);
// apply the pending advance (end of run / before photons are read back) and clear it
hipError_t launch_flush(const PhotonDev &ph, LoopState *st, int blocks, hipStream_t stream);
hipError_t launch_k2e(const double *temp, double *k2e, int M, hipStream_t stream);
// cs_switch: CYCLOSYNCHROTRON_SWITCH -- on, phScattStats and averagePhotonEnergy take the photons with weight != 0 only (mclib.c:1373, :1401)
hipError_t launch_reduce(const PhotonDev &ph, ReducePartial *out, int blocks, int cs_switch, hipStream_t stream);
// struct photon records <-> SoA columns on the device (staging.hip); `aos` is a device buffer of n 176-B records
hipError_t launch_init_states(LoopState *single, LoopState *ranks, int n_ranks, const LoopState &v, hipStream_t stream);
hipError_t launch_convert_comptonized(const PhotonDev &ph, unsigned *converted, hipStream_t stream);   // 'k' with weight != 0 -> 'c' (mcrat_io.c:896-900)
hipError_t launch_clear_slots(const PhotonDev &ph, int first, int count, hipStream_t stream);   // every column zeroed: no list's slots
// rank pool: the per-frame reductions and printPhotons' count for every list (desc[r].len slots from r * stride), one launch
hipError_t launch_rank_reduce(const PhotonDev &ph, int stride, int n_ranks, const RankDesc *desc, ReducePartial *out, int *n_out, int cs_switch,
                              hipStream_t stream);
// mock observations (observe.hip): the photons binned by observer, detection time and energy in one pass over n_slots slots.  The cube and the
// staged inputs are laid out as observe_plan.hpp says; clocks != nullptr: slot i takes its list's clock clocks[i / slots_per_clock] (rank pool),
// else time_now.  The plan has chosen the accumulation path; the adds go on top of what the cube holds (the caller zeroes it).
struct ObservePlan;
struct ObserveDev {
    int n_slots, n_obs, n_t, n_e, n_bins;
    const double *staged;                // cos_obs, sin_obs, cos_lo, cos_hi [n_obs each], t_edges [n_t + 1], e_edges [n_e + 1]
    const double *clocks;
    int slots_per_clock;
    double time_now;
    double *cube;                        // OBSERVE_PLANES planes of n_bins; plane 0 holds 64-bit integer counts
    unsigned long long *n_accepted, *n_outside;   // [n_obs]
};
hipError_t launch_observe(const PhotonDev &ph, const ObserveDev &a, const ObservePlan &plan, bool stokes, int cus, hipStream_t stream);
// line-of-sight optical depths (sightline.hip): n rays marched through the frame hy, one lane per ray.  The block's head -- five status counts and
// the refill form's ray counter -- and the output planes are laid out as sightline_plan.hpp says; the caller zeroes the head and sizes the grid
// (sightline_grid).  ray != nullptr: the caller's rays, seven planes of n doubles (r0, r1, r2, p0, p1, p2, p3); else the n slots of ph.
struct SightlineDev {
    int n;
    double step_frac, h_min;
    int max_steps;
    double tau_stop, surface_level;
    const double *ray;
    unsigned long long *head;            // n_status[5], then the global ray counter
    double *f8;                          // tau, path, surface_r0, surface_r1, surface_r2: n each
    int *i4;                             // steps, status, surface_step: n each
    int refill, own_rays;                // lane refill, and the rays of a workgroup's own range (sightline_own_rays)
};
hipError_t launch_sightline(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const SightlineDev &a, int blocks, hipStream_t stream);
// the radiation field on the hydro mesh (radfield.hip): the n_slots slots of ph located in the frame hy and their moments added per cell or per
// (r, mu) shell.  Head, accumulator and staged edges are laid out as radfield_plan.hpp says; the caller zeroes head and accumulator and sizes the
// grid (radfield_grid).  A bin-major accumulator is turned into the caller's planes by launch_radfield_transpose.
struct RadfieldPlan;
struct RadfieldDev {
    int n_slots, n_r, n_mu, n_bins;
    const double *staged;                // r_edges [n_r + 1], mu_edges [n_mu + 1] (SHELLS)
    unsigned long long *head;            // n_observable, n_unlocated, n_outside
    double *acc;                         // RADFIELD_PLANES words per bin, plane- or bin-major; word 0 holds a 64-bit integer count
};
hipError_t launch_radfield(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const RadfieldDev &a, const RadfieldPlan &plan, int blocks,
                           hipStream_t stream);
hipError_t launch_radfield_transpose(const double *records, double *planes, int n_bins, int cus, hipStream_t stream);
// the comoving radiation field (comoving.hip): the n_slots slots of ph located in the frame hy, boosted into their cell's frame and added per
// (position, fluid-frame energy, fluid-frame cosine) bin.  Head, accumulator and staged edges are laid out as comoving_plan.hpp says; the caller
// zeroes head and accumulator and sizes the grid (comoving_grid).
struct ComovingPlan;
struct ComovingDev {
    int n_slots, n_r, n_mu, n_e, n_a, n_bins;
    const double *staged;                // r_edges [n_r + 1], mu_edges [n_mu + 1] (SHELLS), e_edges [n_e + 1], a_edges [n_a + 1]
    unsigned long long *head;            // n_observable, n_unlocated, n_outside
    double *acc;                         // COMOVING_PLANES planes of n_bins words; plane 0 holds 64-bit integer counts
};
hipError_t launch_comoving(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const ComovingDev &a, const ComovingPlan &plan, int blocks,
                           hipStream_t stream);
// mock observations from any direction on the sky, with images (sky.hip): the photons binned by observer, detection time, energy and, with image
// axes (n_x, n_y >= 1; else both 0), sky-plane position in one pass over n_slots slots.  The cube and the staged inputs are laid out as sky_plan.hpp
// says; clocks as in ObserveDev.  The caller zeroes the cube and the counters and sizes the grid (sky_grid).
struct SkyPlan;
struct SkyDev {
    int n_slots, n_obs, n_t, n_e, n_x, n_y, n_bins;
    const double *staged;                // n0, n1, n2, cos_acc [n_obs each]; (image) x0 .. x2, y0 .. y2 [n_obs each]; t_edges, e_edges; (image) x_edges, y_edges
    const double *clocks;
    int slots_per_clock;
    double time_now;
    double *cube;                        // OBSERVE_PLANES planes of n_bins; plane 0 holds 64-bit integer counts
    unsigned long long *n_accepted, *n_outside;   // [n_obs]
};
hipError_t launch_sky(const PhotonDev &ph, const SkyDev &a, const SkyPlan &plan, bool stokes, int blocks, hipStream_t stream);
// escape-weighted sky observations (escape.hip): the slots an observer accepts compacted into a list, those marched through the frame hy, and the
// list binned by observer, optical depth, detection time, energy and, with image axes, sky-plane position -- three kernels on one stream.  The block
// is laid out as escape_plan.hpp says; the caller zeroes planes, counters and head, copies the staged inputs and the clocks and sizes the three grids.
struct EscapePlan;
struct EscapeDev {
    int n_slots, n_obs, n_tau, n_t, n_e, n_x, n_y, n_bins;
    double step_frac, h_min;
    int max_steps;
    double tau_stop;
    const double *staged;                // sky_plan.hpp's staged inputs, then tau_edges [n_tau + 1]
    const double *clocks;
    int slots_per_clock;
    double time_now;
    double *cube;                        // ESCAPE_PLANES planes of n_bins; plane 0 holds 64-bit integer counts
    unsigned long long *counters;        // n_accepted, n_outside, n_opaque, n_unresolved: [n_obs] each
    unsigned long long *head;            // n_status[5], n_selected, n_observable
    double *tau;                         // the compacted list, room for n_slots entries: the march's tau ...
    int *index, *status;                 // ... the slot, and how the march ended
};
hipError_t launch_escape(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const EscapeDev &a, const EscapePlan &plan, bool stokes,
                         int select_blocks, int march_blocks, int bin_blocks, hipStream_t stream);
// sky observations with a resampling axis and a choice of Stokes frame (resample.hip): observe_sky's pass with a replica axis behind the observer
// and a multiplicity per (photon, replica).  The block and the staged inputs are laid out as resample_plan.hpp says; clocks as in ObserveDev.  The
// caller zeroes the cube and the counters and sizes the grid (resample_grid).  A photon's identity: rank = rank_base + i / rank_stride and slot =
// i % rank_stride for slot i of a pool (rank_stride > 0), rank = rank_base and slot = i otherwise.
struct ResamplePlan;
struct ResampleDev {
    int n_slots, n_obs, n_rep, n_t, n_e, n_x, n_y, n_bins, per_rep;
    int mode, axes;                      // ResampleMode; whether ex and ey are staged
    int slice_reps, n_slices;            // LDS and sliced: the replicas a workgroup's sub-cube holds, and how many such slices the replica axis has
    int grid_x, grid_y;                  // the launch is grid_x * grid_y workgroups: workgroup b walks the slots as number b % grid_x of grid_x, for the slices b / grid_x, + grid_y, ..
    unsigned long long seed;
    int rank_base, rank_stride;
    const double *staged;                // n0, n1, n2, cos_acc [n_obs each]; (axes) x0 .. x2, y0 .. y2 [n_obs each]; t_edges, e_edges; (image) x_edges, y_edges
    const double *clocks;
    int slots_per_clock;
    double time_now;
    double *cube;                        // OBSERVE_PLANES planes of n_bins; plane 0 holds 64-bit integer counts
    unsigned long long *n_accepted, *n_outside, *n_undefined;   // [n_obs]
};
hipError_t launch_resample(const PhotonDev &ph, const ResampleDev &a, const ResamplePlan &plan, bool stokes, int blocks_x, int blocks_y, hipStream_t stream);
// detected-photon event lists (events.hip): the accepted (photon, observer) pairs inside a window of detection time and energy as rows, ordered by
// (observer, rank, slot) or by (observer, key(t_det), rank, slot) -- count, scan, write and, for BY_TIME, a stable radix sort of (key, row) pairs and
// one gather, all on one stream with no host round trip.  The block is laid out as events_plan.hpp says; the caller zeroes the head and copies the
// staged observers and the clocks.  Clocks and a photon's identity as in ResampleDev.
struct EventsPlan;
struct EventsDev {
    int n_slots, n_obs, n_chunks, chunk_slots;
    int order, sky_plane, axes;          // EventsOrder; whether Q and U are carried into the observer's frame; whether ex and ey are staged
    int capacity, n_tiles;               // rows there is room for; tiles of the sort (BY_TIME)
    double t_lo, t_hi, e_lo, e_hi;
    int rank_base, rank_stride;
    const double *staged;                // n0, n1, n2, cos_acc [n_obs each]; (axes) x0 .. x2, y0 .. y2 [n_obs each]
    const double *clocks;
    int slots_per_clock;
    double time_now;
    unsigned long long *n_accepted, *n_outside, *n_undefined;   // [n_obs]
    unsigned long long *offsets;         // [n_obs + 1]; offsets[n_obs]: n_total
    unsigned long long *key_or, *key_nand;   // the OR of all event keys and of all inverted event keys
    unsigned long long *table;           // [n_obs][n_chunks]: the events of a chunk, after the scan the chunk's first row
    int *rank, *slot;                    // the row columns, [capacity] each
    double *t, *e, *w, *s0, *s1, *s2, *s3, *num_scatt, *X, *Y;
    char *type;
    unsigned *sort_table;                // [EVENTS_DIGITS][n_tiles] (BY_TIME, like all that follows)
    unsigned *source;                    // the pool slot behind each unsorted row
    unsigned long long *keys[2];
    unsigned *index[2];
};
hipError_t launch_events(const PhotonDev &ph, const EventsDev &a, const EventsPlan &plan, bool stokes, hipStream_t stream);
// the spectral fit (fit.hip): every row of (count, W) fitted to a cutoff power law or a Band function, one wavefront per spectrum.  The block is laid
// out as fit_plan.hpp says -- FitDev is defined there --; the caller copies the inputs.
struct FitPlan;
struct FitDev;
hipError_t launch_fit(const FitDev &a, const FitPlan &plan, hipStream_t stream);
hipError_t launch_init_states_multi(LoopState *ranks, int n_ranks, const int *open, const double *time_now, const double *remaining, hipStream_t stream);
hipError_t launch_aos_to_soa(const void *aos, const PhotonDev &ph, int n, hipStream_t stream);
// many lists of a rank pool at once: desc = `count` device records {int rank, int n, long long first record in aos}; the rest of each window is cleared
hipError_t launch_pool_aos_to_soa(const void *aos, const PhotonDev &pool, int stride, const void *desc, int count, hipStream_t stream);
hipError_t launch_soa_to_aos(const PhotonDev &ph, void *aos, int first, int n, hipStream_t stream);   // record k = slot first + k
// printPhotons' arrays (mcrat_io.c:137-181): photons with weight != 0, slot order; col: p0-3, comv_p0-3, r0-2, s0-3, num_scatt, weight
struct OutputCols {
    double *col[17];
    char *type;
};
hipError_t launch_output_count(const PhotonDev &ph, int n, unsigned *block_count, unsigned long long *d_total, hipStream_t stream);
hipError_t launch_output_write(const PhotonDev &ph, int n, const int *block_start, const OutputCols &out, hipStream_t stream);

// the cell-lookup grid, built on the device (grid_build.hip) from a GridPlan (hydro_plan.hpp)
hipError_t grid_count(const GridPlan &p, const CellGeom *geom, const CellGeom2 *geom2, int M, unsigned *count, long long nb,
                      unsigned long long *d_total, hipStream_t stream);
size_t grid_scan_scratch_ints(long long nb);
hipError_t launch_exclusive_scan(const unsigned *count, long long n, int *start, int *scratch, long long total, hipStream_t stream);

// photonInjection on the device (inject.hip; mclib.c:9-300)
struct InjectParams {
    int dimensions, geometry;
    double rmin, rmax, theta_min, theta_max;   // the injection slab, mclib.c:34-35,57
    double num_dens_coeff;                     // 8.44f / 20.29f widened (mclib.c:23-32)
    int wien;                                  // spect == 'w'
};
// Poisson photon count of every cell for one weight (mclib.c:87-136); *total receives the sum.  (The same name takes the pool emission's
// arguments below: the two births are one kernel over a rule, inject.hip.)
hipError_t launch_birth_count(const InjectParams &p, const HydroDev &hy, double ph_weight_adjusted, unsigned long long attempt, RngKey key,
                              unsigned *count, unsigned long long *d_total, hipStream_t stream);
// the photons themselves (mclib.c:150-296), ordered by cell then draw, into the SoA columns
hipError_t launch_inject_generate(const InjectParams &p, const HydroDev &hy, double ph_weight_adjusted, RngKey key, const int *start,
                                  const PhotonDev &ph, hipStream_t stream);
// photonInjection for the lists of a rank pool (inject.hip): the slab's cells with the two list-independent factors of mclib.c:110, once per group
// of lists that share the slab, then one workgroup per list
struct alignas(8) InjectSlabCell { int cell; int pad; double v43, g; };
constexpr int POOL_INJECT_CAP = 8192;        // photons one list may receive (LDS table of their cells)
struct alignas(8) PoolInject {
    int inject, group;               // in: takes part; which slab
    unsigned long long seed;         // in
    unsigned stream; int pad;        // in: the list's RNG stream
    double weight_in;                // in: ph_weight
    int min_photons, max_photons;    // in
    double weight_out;               // out
    int n, error;                    // out: photons; 0 ok, 1 no weight fits, 2 no photons, 3 more than the list's window (or the kernel's table) holds
};
// The cells of a region -- Params: InjectParams (the slab) or CsEmitParams (the emission shell, below) -- flagged, flag[i] = 1, and counted; waits.
template <class Params>
hipError_t launch_region_flag(const Params &p, const HydroDev &hy, unsigned *flag, unsigned long long *d_total, int *n_cells, hipStream_t stream);
// ... and, the flags scanned into `start`, their records in cell order (n_cells == 0: nothing to write)
hipError_t launch_region_write(const InjectParams &p, const HydroDev &hy, const unsigned *flag, int n_cells, int *start, int *scratch, InjectSlabCell *out,
                               hipStream_t stream);
hipError_t launch_inject_pool(const InjectParams &p, const HydroDev &hy, const PhotonDev &pool, int stride, int n_ranks, const InjectSlabCell *slab, int n_slab,
                              PoolInject *lists, int group, hipStream_t stream);
// getHydroData on the device (ingest.hip; mcrat_io.c:1898-1990); SlabDev, ChomboBox and StagePartial: hydro_plan.hpp
struct HydroCols {          // struct hydro_dataframe's columns (mcrat.h:194-244), device arrays of M doubles
    double *r0, *r1, *r2, *s0, *s1, *s2;
    double *v0, *v1, *v2;
    double *dens, *dens_lab, *pres, *temp, *gamma;
    double *r, *theta;
    double *B0, *B1, *B2;   // magnetic field (B_FIELD_CALC == SIMULATION; mcrat_hip_set_hydro_extras)
};
struct FlashDev {           // device copies of a FLASH checkpoint's datasets (mclib_flash.c:143-193)
    const double *coord, *bsize;
    const int *node;
    const double *velx, *vely, *dens, *pres;
    int coord_stride, bsize_stride;
    long long n_blocks;
    double L, D, P;
};
struct PlutoDev {           // device copies of readGridFile's arrays and the .dbl variable blocks
    int nx, ny, nz;
    const double *x1, *dx1, *x2, *dx2, *x3, *dx3;
    const double *rho, *vx1, *vx2, *vx3, *prs;
    double L, D, P;
};
struct ChomboDev {
    const ChomboBox *boxes;
    int n_boxes;
    long long cells;
    const double *data;
    const double *x[3], *dx[3];        // per axis: the levels' x*_array / dx*_array (mclib_pluto.c:446-517), concatenated
    const unsigned char *covered;      // good_node_buffer == 0 (:206-345); null when the mask is not consulted
    int kv[5];                         // component index of rho, vx1, vx2, vx3, prs (-1: absent)
    double L, D, P;
};
hipError_t ingest_count_chombo(const ChomboDev &h, const SlabDev &slab, unsigned *block_count, unsigned long long *d_total, hipStream_t stream);
hipError_t ingest_write_chombo(const ChomboDev &h, const SlabDev &slab, const int *block_start, const HydroCols &out, hipStream_t stream);
// marks the cells of boxes [c0, c1) that a box of [f0, f1) (the next finer level) covers
hipError_t launch_chombo_mask(const ChomboBox *boxes, int c0, int c1, int f0, int f1, int ref_ratio, int three, unsigned char *covered, hipStream_t stream);
// phAbsCyclosynch (mc_cyclosynch.c:1571-1623) on the device (staging.hip): photons at or below their cell's cyclotron frequency and
// all pool photons become null slots (setNullPhoton, photons.c:210-250)
struct CsParams {
    int dimensions, b_field_calc;
    double epsilon_b;
};
struct CsAbsPartial { double abs_weight; int abs_count, scatt_count; };      // one per workgroup
int cs_absorb_blocks(int n);
hipError_t launch_cs_absorb(const CsParams &p, const PhotonDev &ph, const double *temp, const HydroCols &h, CsAbsPartial *partials, hipStream_t stream);
struct OutflowDev {
    int simulation_type;
    double gamma_infinity, lumi, r00, t_comov, ddensity, theta_j, p;
};
long long ingest_blocks(long long n_virtual);   // workgroups (and block_count entries) of the two selection passes
hipError_t ingest_count_flash(const FlashDev &f, const SlabDev &slab, unsigned *block_count, unsigned long long *d_total, hipStream_t stream);
hipError_t ingest_write_flash(const FlashDev &f, const SlabDev &slab, const int *block_start, const HydroCols &out, hipStream_t stream);
hipError_t ingest_count_pluto(const PlutoDev &g, const SlabDev &slab, unsigned *block_count, unsigned long long *d_total, hipStream_t stream);
hipError_t ingest_write_pluto(const PlutoDev &g, const SlabDev &slab, const int *block_start, const HydroCols &out, hipStream_t stream);
hipError_t launch_fill_spherical(int dims, int geom, const HydroCols &h, int M, hipStream_t stream);
hipError_t launch_outflow_prep(int dims, int geom, const OutflowDev &o, const HydroCols &h, int M, hipStream_t stream);
int stage_cells_blocks(int M);
hipError_t launch_stage_cells(int dims, int geom, const HydroCols &h, int M, CellGeom *og, CellGeom2 *og2, CellFluid *of, double *ofc, double *otemp,
                              double *ogamma, StagePartial *partials, double *samples, int stride, int nsamp, hipStream_t stream);
// createHotCrossSection on the device (hot_table.hip; hot_x_section.c:82-133,324-400)
constexpr int HOT_TABLE_SUBSTREAMS = 256;   // sample k of an entry belongs to substream k % 256 (part of the table's definition)
struct HotTableParams {
    int n_ph_e, n_t;
    double log_ph_e_min, log_ph_e_max, log_t_min, log_t_max;
    long long calls;
    unsigned long long seed;
};
hipError_t launch_hot_table(const HotTableParams &p, double *table, hipStream_t stream);
// photonEmitCyclosynch, inject_single_switch == 0, on the device (inject.hip; mc_cyclosynch.c:1200-1460)
struct CsEmitParams {
    int dimensions, geometry, b_field_calc;
    double epsilon_b;
    double rmin, rmax, theta_min, theta_max;        // the shell of :1203-1204 and the thread's angle range
};
struct CsHookArgs { CsEmitParams p; HydroCols h; };      // (see launch_rank_loop)
// d_flags[0] counts cells whose integral ran out of intervals, and on attempt 0 [1] the cells of the shell, [2] the cells past QAGS' first rule
hipError_t launch_birth_count(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, double ph_weight_adjusted, unsigned long long attempt,
                              RngKey key, unsigned *count, unsigned long long *d_total, unsigned *d_flags, hipStream_t stream);
hipError_t launch_cs_emit_generate(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, double ph_weight_adjusted, RngKey key, const int *start,
                                   int n_emit, const int *null_slots, const PhotonDev &ph, hipStream_t stream);
// the hook of mcrat.c:786-808 after every pass of a cyclo-synchrotron frame (one workgroup on the context's stream) and the state it
// keeps on the device, so that the host reads a frame's progress back once per batch of passes: when the hook needs the host (the list
// has no null slot left; the rebinning is due) it parks the loop -- LoopState::done = LOOP_CS_HALT makes the step and event kernels of
// the passes already queued return at once -- and says why in `halt`
constexpr int LOOP_CS_HALT = 3;      // LoopState::done value
constexpr int CS_HALT_GROW = 1;      // nothing was done for this pass: double the list, launch the hook again with resume = 1
constexpr int CS_HALT_REBIN = 2;     // the pass is complete; rebinCyclosynchCompPhotons is due (mcrat.c:797-808)
constexpr int CS_HALT_HOOK = 3;      // rank pool, hook-kernel form: rank_loop_kernel parked the list after a pass the hook has to look at (cs_replace_pool_kernel)
struct CsFrame {
    int halt;
    int saved_done;                  // LoopState::done as the pass left it
    int emitted;                     // replacements since the host last looked (num_cyclosynch_ph_emit)
    int scatt_num;                   // scatt_cyclosynch_num_ph
    int max_photons;
    int pad;
    unsigned long long last_iteration;   // LoopState::iteration of the last pass the hook handled (queued passes after `done` are no-ops)
    double n_comptonized;            // mcrat.c:788, summed in pass order
};
hipError_t launch_cs_replace(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, RngKey key, LoopState *st, const PhotonDev &ph,
                             CsFrame *frame, int resume, hipStream_t stream);
// pool emission for the lists of a rank pool (inject.hip): the emission shell's cells with what photonEmitCyclosynch computes per cell, once per
// group of lists that share the shell, then one workgroup per list
struct alignas(8) CsShellCell { int cell; int pad; double integral; double volume; };
struct alignas(8) CsPoolEmit {
    int open, group;                 // in: takes part; which shell it emits into
    unsigned long long seed;         // in: the list's emission seed
    double weight_in, max_photons;   // in: ph_weight_suggest; rebin_e_perc * maximum_photons
    double weight_out;               // out: the adjusted weight
    int n_emit, error;               // out: photons emitted; 0 ok, 1 no weight fits, 2 fewer null slots than photons, 3 the list would outgrow its
                                     //      window of the pool, 4 more photons than the kernel's tables hold
};
// the shell's cells: launch_region_flag, then their records; *not_converged: the cells whose integral ran out of intervals (0 for an empty shell)
hipError_t launch_region_write(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, const unsigned *flag, int n_cells, int *start, int *scratch,
                               CsShellCell *out, unsigned *not_converged, hipStream_t stream);
hipError_t launch_cs_emit_pool(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, const PhotonDev &pool, int stride, int n_ranks, RankDesc *desc,
                               const CsShellCell *shell, int n_shell, CsPoolEmit *lists, int group, hipStream_t stream);
// phAbsCyclosynch for the open lists of a rank pool, one workgroup per list (staging.hip)
hipError_t launch_cs_absorb_pool(const CsParams &p, const PhotonDev &pool, int stride, int n_ranks, const RankDesc *desc, const int *open, const double *temp,
                                 const HydroCols &h, CsAbsPartial *per_list, hipStream_t stream);
// the hook for every parked list of a rank pool (one workgroup per list; a list out of null slots doubles inside its window of the pool)
hipError_t launch_cs_replace_pool(const CsEmitParams &p, const HydroDev &hy, const HydroCols &h, LoopState *states, const PhotonDev &pool, int stride,
                                  int n_ranks, RankDesc *desc, CsFrame *frames, hipStream_t stream);
// the list's null slots in ascending order (addToPhotonList's null_ph_indexes, photons.c:181-189): count per 256 slots, then write
hipError_t launch_null_count(const PhotonDev &ph, unsigned *block_count, unsigned long long *d_total, hipStream_t stream);
hipError_t launch_null_write(const PhotonDev &ph, const int *block_start, int *null_slots, hipStream_t stream);
// slots [first, first + count) become null photons (reallocatePhotonListMemory, photons.c:72-78)
hipError_t launch_null_fill(const PhotonDev &ph, int first, int count, hipStream_t stream);
// rebinCyclosynchCompPhotons on the device (inject.hip; mc_cyclosynch.c:246-712)
int rebin_range_blocks(int n);
hipError_t launch_rebin_range(const PhotonDev &ph, int three, RebinRange *partials, hipStream_t stream);
// bin of every slot (-1: not rebinned; -2: outside the histograms, the reference's exit(1)) and the number of slots per bin
hipError_t launch_rebin_assign(const PhotonDev &ph, const RebinAxes &ax, int *bin_of, unsigned *bin_count, hipStream_t stream);
// slots of each bin (bin_start from the scan of bin_count); then one thread per bin: the weighted sums in slot order and the
// rebinned photon as a record (create_rebinned_photons :504-607)
hipError_t launch_rebin_fill(const PhotonDev &ph, const int *bin_of, const int *bin_start, unsigned *cursor, int *members, hipStream_t stream);
struct RebinRec {              // one rebinned photon (or an empty bin: valid == 0)
    double weight, p0, p1, p2, p3, r0, r1, r2, s0, s1, s2, s3, num_scatt;
    int valid, pad;
};
hipError_t launch_rebin_create(const PhotonDev &ph, const RebinAxes &ax, const int *bin_start, int *members, RebinRec *recs,
                               unsigned *empty_bins, hipStream_t stream);
// after the old photons are nullified: record b into the b-th null slot (addToPhotonList, photons.c:190-199)
hipError_t launch_rebin_place(const PhotonDev &ph, const RebinRec *recs, int total_bins, const int *null_slots, hipStream_t stream);
// setNullPhoton for every 'k' and 'c' photon (:573-581)
hipError_t launch_rebin_nullify(const PhotonDev &ph, hipStream_t stream);
// the rebinning of many lists of a rank pool in two launches, one workgroup per list (inject.hip, rebin_pool_kernel)
struct RebinPoolList {
    int first, n;              // the list's window in the pool's slots
    RebinAxes ax;              // (second launch) the histograms, fixed by the host from the first launch's ranges
    unsigned long long scratch;   // byte offset of the list's scratch (rebin_pool_scratch_bytes) in the buffer handed to the second launch
    int status;                // out: 0 rebinned; 1 a photon maps outside the histograms (list untouched); 2 fewer null slots than bins
    int empty_bins, n_null;    // out
    int pad;
};
size_t rebin_pool_scratch_bytes(int n, int total_bins);
hipError_t launch_rebin_pool_range(const PhotonDev &pool, int three, const RebinPoolList *lists, int n_lists, RebinRange *out, hipStream_t stream);
hipError_t launch_rebin_pool(const PhotonDev &pool, RebinPoolList *lists, int n_lists, char *scratch, hipStream_t stream);
hipError_t grid_build(const GridPlan &p, const CellGeom *geom, const CellGeom2 *geom2, const CellFluid *fluid, const double *fluid_c, int M,
                      unsigned *count, int *start, int *scan_scratch, int *entries, FatCell *cells, BucketDir *dir, int *covered, long long nb,
                      long long total, hipStream_t stream);      // covered: the covered-octant table, or nullptr where the grid has none
hipError_t launch_lookup(const KernelConfig &kc, const HydroDev &hy, int n, const double *a0, const double *a1,
                         const double *a2, int *out, hipStream_t stream);
// The launchers that every kernels translation unit (kernels.hip: one per TAU_CALCULATION and DIMENSIONS) defines for itself; launchers.hip picks the
// unit's table and calls through it.
struct TuLaunchers {
    decltype(&launch_step) step;
    decltype(&launch_event) event;
    decltype(&launch_tape_pass) tape_pass;
    decltype(&launch_rank_loop) rank_loop;
    decltype(&launch_rank_loop_tape) rank_loop_tape;
    decltype(&launch_sc_propose) sc_propose;
    decltype(&launch_sc_resolve) sc_resolve;
    decltype(&launch_fast_frame) fast_frame;
};
// physics.hpp's functions on arrays (functions.hip; mcrat_hip_eval_function)
// (hy: the context's cross-section table for THERMAL_CROSS_SECTION; kc: STOKES, and DIMENSIONS / geometry for HYDRO_COORDS)
hipError_t launch_eval_function(const KernelConfig &kc, const HydroDev &hy, int fn, int n, const double *in, double *out, uint64_t seed, uint32_t stream_id,
                                hipStream_t stream);

}  // namespace mcrat
