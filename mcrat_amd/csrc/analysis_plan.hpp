// analysis_plan.hpp -- the three host rules that the analysis products' entry points share (engine.hip, "the analysis products' device blocks" and
// on): where a call's photons come from, the order in which the sky family's observer inputs are staged, and whose staged hydro frame a product may
// read.  Plain inline C++ -- no HIP call, no context -- so that a CPU test can drive them (tests/test_analysis_plan_cpu.py).  Only engine.hip
// includes it.
#pragma once
#include <vector>
#include "sky_plan.hpp"

namespace mcrat {

// ------------------------------------------------------------------ where the photons come from
// The slots a product reads and what its kernel is told of them (launch.hpp: ObserveDev, SkyDev, EscapeDev, ResampleDev, EventsDev).  clocks: one
// per slots_per_clock slots (a rank pool's lists, host memory), or nullptr and time_now for all.  A photon's identity is rank = rank_base +
// i / rank_stride and slot = i % rank_stride for slot i of a pool (rank_stride > 0), rank = rank_base and slot = i otherwise.
struct PhotonSource {
    int n_slots;
    const double *clocks;
    int n_clocks, slots_per_clock;
    double time_now;
    int rank_base, rank_stride;
};
// one list -- a stand-alone context (view_rank 0) or the view of a pool's list view_rank -- at its clock time_now
inline PhotonSource list_source(int n_slots, double time_now, int view_rank) { return PhotonSource{n_slots, nullptr, 0, 1, time_now, view_rank, 0}; }
// every slot of a pool of n_ranks lists, rank_stride slots apart, list r at clocks[r]
inline PhotonSource pool_source(int n_slots, int n_ranks, int rank_stride, const double *clocks) { return PhotonSource{n_slots, clocks, n_ranks, rank_stride, 0.0, 0, rank_stride}; }

// ------------------------------------------------------------------ the order in which an observer's inputs are staged
// What the kernels of sky.hip, escape.hip, resample.hip and events.hip read at `staged` (the comments in launch.hpp restate it), appended to *in:
//     n0, n1, n2, cos_acc [n_obs each];  axes: x0, x1, x2, y0, y1, y2 [n_obs each];
//     edges: t_edges [n_t + 1], e_edges [n_e + 1] and, behind them, image: x_edges [n_x + 1], y_edges [n_y + 1]
// A sky observation has axes exactly with an image, and edges; an escape-weighted one the same, and its caller appends tau_edges [n_tau + 1]; a
// resampled one may have axes without an image (STOKES_SKY_PLANE); an event list has the vectors only.  What is appended is the plan's
// staged_doubles, for escape without the n_tau + 1.  The lists' clocks are no part of it: the callers put them where their block keeps them.
inline void stage_observer_inputs(const SkyArgs &s, bool axes, bool edges, bool image, std::vector<double> *in)
{
    const size_t n_obs = (size_t)s.n_obs;
    for (const double *v : {s.n0, s.n1, s.n2, s.cos_acc}) in->insert(in->end(), v, v + n_obs);
    if (axes)
        for (const double *v : {s.x0, s.x1, s.x2, s.y0, s.y1, s.y2}) in->insert(in->end(), v, v + n_obs);
    if (!edges) return;
    in->insert(in->end(), s.t_edges, s.t_edges + s.n_t + 1);
    in->insert(in->end(), s.e_edges, s.e_edges + s.n_e + 1);
    if (!image) return;
    in->insert(in->end(), s.x_edges, s.x_edges + s.n_x + 1);
    in->insert(in->end(), s.y_edges, s.y_edges + s.n_y + 1);
}

// ------------------------------------------------------------------ whose staged hydro frame a product reads
// A product of context c reads the frame staged on h: c itself (same), or another context with the same switches on the same device.
struct FrameSwitches { int dimensions, geometry, table, device; };       // DIMENSIONS, GEOMETRY, TAU_CALCULATION == TABLE, the device's index
enum FrameVerdict { FRAME_OK = 0, FRAME_MISMATCH, FRAME_NONE, FRAME_NO_TABLE };
// In this order: the switches -- `table` among them only for a product that marches through the frame (with_table: sightlines, escape) --; the
// frame, with M > 0 cells for a product that sums per cell (need_cells: the two fields); with_table and c has TAU_CALCULATION == TABLE: the hot
// cross-section table that h's frame came with.
inline FrameVerdict frame_verdict(const FrameSwitches &c, const FrameSwitches &h, bool same, bool have_hydro, int M, bool hot_table, bool with_table, bool need_cells)
{
    if (!same && (h.dimensions != c.dimensions || h.geometry != c.geometry || (with_table && h.table != c.table) || h.device != c.device)) return FRAME_MISMATCH;
    if (!have_hydro || (need_cells && M <= 0)) return FRAME_NONE;
    if (with_table && c.table && !hot_table) return FRAME_NO_TABLE;
    return FRAME_OK;
}

}  // namespace mcrat
