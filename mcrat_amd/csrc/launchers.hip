// launchers.hip -- the launchers of launch.hpp whose kernels are built per TAU_CALCULATION and DIMENSIONS: route to the translation unit that holds
// them (see the head of kernels.hip), through the table of launchers each unit defines (launch.hpp, TuLaunchers).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "rng.hpp"

namespace mcrat {

namespace tau_direct_d0 { const TuLaunchers &launchers(); }
namespace tau_direct_d1 { const TuLaunchers &launchers(); }
namespace tau_direct_d2 { const TuLaunchers &launchers(); }
namespace tau_table_d0 { const TuLaunchers &launchers(); }
namespace tau_table_d1 { const TuLaunchers &launchers(); }
namespace tau_table_d2 { const TuLaunchers &launchers(); }

static const TuLaunchers *unit_of(const KernelConfig &kc)
{
    static const TuLaunchers *const units[2][3] = {{&tau_direct_d0::launchers(), &tau_direct_d1::launchers(), &tau_direct_d2::launchers()},
                                                   {&tau_table_d0::launchers(), &tau_table_d1::launchers(), &tau_table_d2::launchers()}};
    static_assert(DIM_TWO == 0 && DIM_TWO_POINT_FIVE == 1 && DIM_THREE == 2, "the units' order");
    return (kc.dimensions >= DIM_TWO && kc.dimensions <= DIM_THREE) ? units[kc.table ? 1 : 0][kc.dimensions] : nullptr;
}
#define MCRAT_ROUTE(member, ...) do { const TuLaunchers *unit = unit_of(kc); return unit ? unit->member(__VA_ARGS__) : hipErrorInvalidValue; } while (0)

int step_grid_blocks(int n_pad)
{
    const int pairs = n_pad / 2;
    int blocks = (pairs + STEP_BLOCK - 1) / STEP_BLOCK;
    // all workgroups resident at once: every workgroup streams its chunks back to back and pays the
    // latency-bound slow path once.  MCRAT_HIP_STEP_BLOCKS overrides the cap (tuning).
    int cap = 768;                        // 3 workgroups per CU, all resident at the kernel's register budget
    if (const char *e = getenv("MCRAT_HIP_STEP_BLOCKS")) { const int v = atoi(e); if (v > 0) cap = v; }
    if (blocks > cap) {                   // balance: every workgroup gets the same number of chunks
        const int per_block = (blocks + cap - 1) / cap;
        blocks = (blocks + per_block - 1) / per_block;
    }
    if (blocks < 1) blocks = 1;
    return blocks;
}

hipError_t launch_step(const KernelConfig &kc, bool force_relocate, const PhotonDev &ph, const HydroDev &hy,
                       LoopState *st, RngKey key, Cand *block_min, int blocks, Shortlist *sl, hipStream_t stream)
{
    MCRAT_ROUTE(step, kc, force_relocate, ph, hy, st, key, block_min, blocks, sl, stream);
}

hipError_t launch_event(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, RngKey key,
                        const Cand *block_min, int n_blocks, Shortlist *sl, hipStream_t stream)
{
    MCRAT_ROUTE(event, kc, ph, hy, st, key, block_min, n_blocks, sl, stream);
}

hipError_t launch_tape_pass(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, RngKey key, const TapeDev &tape,
                            Cand *block_min, int n_blocks, Shortlist *sl, hipStream_t stream)
{
    MCRAT_ROUTE(tape_pass, kc, ph, hy, st, key, tape, block_min, n_blocks, sl, stream);
}

hipError_t launch_rank_loop(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *states, RngKey key, const RankLaunch &rl,
                            hipStream_t stream)
{
    MCRAT_ROUTE(rank_loop, kc, ph, hy, states, key, rl, stream);
}

hipError_t launch_rank_loop_tape(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *states, RngKey key, int n_ranks, int rank_stride,
                                 const RankDesc *desc, const double *u, TapeList *tapes, long long max_passes, hipStream_t stream)
{
    MCRAT_ROUTE(rank_loop_tape, kc, ph, hy, states, key, n_ranks, rank_stride, desc, u, tapes, max_passes, stream);
}

hipError_t launch_sc_propose(const KernelConfig &kc, bool force_relocate, const PhotonDev &ph, const HydroDev &hy, LoopState *st,
                             ScState *sc, RngKey key, Cand *block_min, int blocks, Shortlist *sl, ScProposal *out, const ScFold &fold, hipStream_t stream)
{
    MCRAT_ROUTE(sc_propose, kc, force_relocate, ph, hy, st, sc, key, block_min, blocks, sl, out, fold, stream);
}

hipError_t launch_sc_resolve(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, LoopState *st, ScState *sc, RngKey key,
                             const ScProposal *all, int world, const ScFold &fold, hipStream_t stream)
{
    MCRAT_ROUTE(sc_resolve, kc, ph, hy, st, sc, key, all, world, fold, stream);
}

hipError_t launch_fast_frame(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, RngKey key, double remaining_time, int windows,
                             int max_passes, FastCounts *counts, const FastLists &lists, hipStream_t stream)
{
    MCRAT_ROUTE(fast_frame, kc, ph, hy, key, remaining_time, windows, max_passes, counts, lists, stream);
}

}  // namespace mcrat
