// rank_form_plan.hpp -- the launch form of rank_loop_kernel (kernels.hip): which builds of the kernel exist, which of them a launch request resolves
// to and with how much LDS, the grid of a queue launch, and the engine's choice of threads per list.  Plain inline C++ -- no HIP call, no context, no
// environment -- so that a CPU test can drive every rule (tests/test_rank_form_plan_cpu.py) and the engine can ask before it launches.
#pragma once
#include <stddef.h>
#include "device_types.hpp"

namespace mcrat {

#ifndef RANK_SMALL
#define RANK_SMALL 128                 // threads of the small workgroup (a request for 128); -DRANK_SMALL=64 for the A/B of one-wave lists
#endif
constexpr int RANK_COLUMNS_GLOBAL = 1 << 30;      // longest_list of lists that change length: no list is short enough for LDS

// Bytes of LDS per slot of a list whose per-pass columns are resident: with 256 threads r, u, -1/tau, idx and the flag byte; otherwise only r and
// -1/tau (idx, flags and u stay in HBM/L2).  rank_loop_kernel asserts that its column layout (Cols::lds_bytes_per_slot) says the same.
constexpr int rank_lds_bytes_per_slot(int block) { return block == 256 ? 7 * (int)sizeof(double) + (int)sizeof(int) + 1 : 4 * (int)sizeof(double); }
// The longest list whose per-pass columns go to LDS, which is also the PITCH of the LDS copy's columns -- a constant of the build, so that the kernel
// reaches a slot's columns through immediate offsets (photon_cols.hpp, ListCols) -- and therefore what every resident launch asks for:
//   256 threads   two lists per CU: 13 KB of static LDS and 61 B per slot each within 160 KB -> 1088 slots (2 x (13 024 + 66 368) = 158 784 B)
//   128 threads   four per CU: 7 KB of static LDS and 32 B per slot each: 1024 slots
//   512 threads   lists of thousands of photons, one list per CU: 27 KB of static LDS and 32 B per slot within 160 KB -> 4096 slots
constexpr int rank_lds_limit(int block) { return block == 128 ? 1024 : (block == 512 ? 4096 : 1088); }
// (static LDS of the resident builds: 13 024 / 6 736 / 25 616 B at 256 / 128 / 512 threads, the same in every such instantiation, DIRECT and TABLE --
// profiles/column_addressing_kernel_resources.txt; the compiler's occupancy figure knows nothing of the dynamic part, this does)
static_assert(2 * (13024 + rank_lds_limit(256) * rank_lds_bytes_per_slot(256)) <= 160 * 1024 &&
              4 * (6736 + rank_lds_limit(128) * rank_lds_bytes_per_slot(128)) <= 160 * 1024 &&
              25616 + rank_lds_limit(512) * rank_lds_bytes_per_slot(512) <= 160 * 1024, "the lists per CU of each form fit the CU's LDS at the full pitch");

// Which builds of rank_loop_kernel exist -- per (DIMS, GEOM, STOKES) and TAU_CALCULATION -- and why not the others (456 instantiations, 53 MB of
// device code, minutes per translation unit; every form costs 36 of them):
//   tape     256 threads, columns in HBM/L2, no fused pass, no hook, no queue: a validation mode, one launch form for every list length.
//   hook     (CSH, the cyclo-synchrotron hook inside the loop) 64, RANK_SMALL or 256 threads; lists that change length: columns in HBM/L2, no fused
//            pass, no queue (such lists go to the host between passes: one frame per launch).  64 threads -- one wavefront per list, eight lists per
//            CU: every resident wave is always at work (no barrier waits) -- exist with the hook only.
//   fused    where rank_block_rule can ask for it: DIRECT optical depths, not in spherical geometry (there it measured slower), 256 or
//            512 threads (128: it measured no gain on thin frames, round 2).  Everything else has the queue form of a pass only.
//   queue    256-thread lists with their columns in LDS, with or without the fused pass: carrying the queue's paths costs a build registers (see
//            rank_loop_kernel); every other launch form runs a plan frame by frame (engine.hip, mcrat_hip_pool_run_frames).
//   the rest RANK_SMALL, 256 or 512 threads, columns in LDS or in HBM/L2.
constexpr bool rank_build_exists(int geom, bool table, bool resident, int threads, bool fuse, bool hook, bool queue, bool tape)
{
    if (tape) return threads == 256 && !resident && !fuse && !hook && !queue;
    if (hook) return (threads == 64 || threads == RANK_SMALL || threads == 256) && !resident && !fuse && !queue;
    if (fuse && (table || geom == GEOM_SPHERICAL || (threads != 256 && threads != 512))) return false;
    if (queue) return threads == 256 && resident;
    return threads == RANK_SMALL || threads == 256 || threads == 512;
}

// A launch's form: the template arguments of rank_loop_kernel that are chosen at run time.
struct RankForm { bool stokes, resident; int threads; bool fuse, hook, queue; };
// What a launch asks for ...
struct RankFormRequest {
    int threads;          // per list: 64 (with the hook only), 128, 256 or 512; anything else runs 256
    bool fuse;            // the build with the fused pass, where one exists; unfused where not
    bool hook;            // cyclo-synchrotron lists with the hook inside the loop
    bool queued;          // a frame-queue launch
    int longest_list;     // sizes the LDS copy of the per-pass columns; RANK_COLUMNS_GLOBAL: the columns stay in HBM/L2
    bool stokes;
    int geometry;
    bool table;           // TAU_CALCULATION == TABLE
    bool no_lds_lists;    // MCRAT_HIP_NO_LDS_LISTS is set (to anything): the columns stay in HBM/L2
};
// ... and what it gets
struct RankFormPlan {
    RankForm form;
    int lds_slots;        // slots the lists occupy of the per-pass columns in LDS (0: in HBM/L2)
    size_t dyn_bytes;     // ... and the bytes of LDS those slots hold: what a resident list copies in and out
    bool no_queue_build;  // a queued request whose form has no queue build: the plan runs frame by frame
    size_t lds_bytes;     // the launch's dynamic LDS: the columns lie rank_lds_limit slots apart whatever the lists' length, so the limit's bytes
};
inline RankFormPlan rank_form_resolve(const RankFormRequest &q)
{
    RankFormPlan p{RankForm{q.stokes, false, 256, false, q.hook, q.queued}, 0, 0, false, 0};
    // threads per list: an unknown count runs 256 (64 is known with the hook only, 512 without it only)
    const int block = (q.threads == 128 || (q.threads == 64 && q.hook) || (q.threads == 512 && !q.hook)) ? q.threads : 256;
    p.form.threads = block == 128 ? RANK_SMALL : block;
    if (!q.hook) {
        // per-pass columns in LDS for lists of up to rank_lds_limit photons
        if (!q.no_lds_lists && q.longest_list <= rank_lds_limit(block)) p.lds_slots = (q.longest_list + 15) & ~15;
        p.form.resident = p.lds_slots > 0;
    }
    p.dyn_bytes = (size_t)p.lds_slots * rank_lds_bytes_per_slot(block);
    // (by the BUILD's thread count, as the kernel takes its pitch: with -DRANK_SMALL=64 a request for 128 runs the 64-thread build)
    p.lds_bytes = p.form.resident ? (size_t)rank_lds_limit(p.form.threads) * rank_lds_bytes_per_slot(p.form.threads) : 0;
    // a fused request where no fused build exists runs unfused
    p.form.fuse = q.fuse && rank_build_exists(q.geometry, q.table, p.form.resident, p.form.threads, true, q.hook, q.queued, false);
    p.no_queue_build = q.queued && !rank_build_exists(q.geometry, q.table, p.form.resident, p.form.threads, p.form.fuse, q.hook, true, false);
    return p;
}

// Workgroups of a queue launch: persistent, as many as the device holds at once (they are dealt to the XCDs round-robin, an eighth each) -- more
// would only start, find their queue empty and leave -- and at most one per open item; n_open where the runtime would not say what a CU holds.
inline int rank_queue_grid(int n_open, int per_cu, int cus) { return (per_cu > 0 && cus > 0 && per_cu * cus < n_open) ? per_cu * cus : n_open; }

// Threads per list and the fused pass, as the engine picks them once per frame.  MCRAT_HIP_RANK_BLOCK / MCRAT_HIP_RANK_FUSE as atoi reads them
// (set to 0 is not unset: a block of 0 runs 256 threads, a fuse of 0 switches the fused pass off).
struct RankBlock { int threads; bool fuse; };
struct RankEnv { bool block_set = false; int block = 0; bool fuse_set = false; int fuse = 0; };

// Lists per CU is what the virtual-rank kernel's throughput hangs on (kernels.hip), so many lists get 128-thread workgroups, four to a CU -- unless
// there are too few lists to fill the device that way, or the lists are too long to keep in LDS, or the frames are optically thin: a thin frame is a
// dozen passes in which half the photons change cell, i.e. slow-path throughput per list, and there 256 threads per list do better.  The engine
// cannot know the optical depth before it has run a frame; it looks at the previous one (passes_per_list).
inline RankBlock rank_block_rule(int n_ranks, int cus, int longest_list, double passes_per_list, int geometry, const RankEnv &env)
{
    RankBlock b;
    if (env.block_set) {
        // (an override asks for the fused pass in spherical geometry too; rank_form_resolve drops it there)
        b.threads = env.block == 128 ? 128 : (env.block == 512 ? 512 : 256);
        b.fuse = passes_per_list < 48.0;
    } else {
        const bool many = n_ranks > 2 * cus && longest_list <= 1024;
        // ... and, whatever the frame looks like, when there are many times more lists than the device holds at once: four lists per CU then
        // overlap one list's walk with the others' passes all the time (10 246 lists, thin frames: cfg2 5.70 -> 4.96 ms, cfg3 8.44 -> 7.08 ms;
        // 4098 lists 2.50 -> 2.32 ms; 2049 lists no difference; 1025 lists 0.83 -> 0.85 ms)
        const bool very_many = n_ranks >= 12 * cus && longest_list <= 1024;
        b.threads = ((many && passes_per_list >= 48.0) || very_many) ? 128 : 256;
        // lists of thousands of photons (sample_mc.par:21-22 allows 5000 per rank) of which there are about as many as CUs, or fewer: a list has its
        // CU to itself whatever the workgroup size, so it gets 512 threads -- a pass takes half the trips (200 lists of 5000 photons, cfg2: 5.2 -> ms)
        if (longest_list > 1088 && n_ranks <= cus + cus / 4) b.threads = 512;
        // the build with the fused pass (kernels.hip, rank_loop_kernel<.., FUSE>) for frames that looked optically thin last time (or
        // have not been seen yet): there most slots change cell between two events
        // (not in spherical geometry: two slots' acos / atan2 side by side cost the fused build 50 B of scratch per lane, and the spherical
        // benchmark frames run 2 % faster without it -- cfg3 at 1e7 photons 8.62 -> 8.43 ms; the cylindrical Stokes frame 1.07 -> 0.94 ms with it)
        b.fuse = passes_per_list < 48.0 && geometry != GEOM_SPHERICAL;
    }
    if (env.fuse_set) b.fuse = env.fuse != 0;
    return b;
}

// The cyclo-synchrotron pool's lists change length: their columns stay in HBM/L2, so LDS does not limit the lists per CU; with more than two lists
// per CU the 128-thread workgroups put four on one (cfg5 at 1e7 photons: 420 -> 380 ms per frame) ...
inline RankBlock cs_rank_block_rule(int n_ranks, int cus, bool hook_kernel, const RankEnv &env)
{
    RankBlock b{n_ranks > 2 * cus ? 128 : 256, false};
    // ... and with eight and more per CU one wavefront per list (eight on a CU): no wave ever waits at a barrier for the one that walks
    // the event (cfg5: 250 -> 230 ms per frame); only with the hook inside the loop (the hook kernel is written for 128 threads and more)
    if (n_ranks > 8 * cus && !hook_kernel) b.threads = 64;
    if (env.block_set) b.threads = env.block == 64 ? 64 : (env.block == 128 ? 128 : 256);
    return b;
}

}  // namespace mcrat
