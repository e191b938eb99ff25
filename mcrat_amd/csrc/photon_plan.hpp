// photon_plan.hpp -- where the photons live: the host's rules for the photon storage (engine.hip), as plain functions.
//
// Every kernel trusts the PhotonDev the host hands it, so what decides where the kernels read and write is kept here, once, and checked on the
// CPU (tests/test_photon_plan_cpu.py):
//   the column tables   PhotonDev's 24 double columns in PhotonCol order (photon_cols.hpp; engine.hip ties the two with one static_assert per
//                       column); the first 19 cross the ABI, and a second table names the ABI's member for each of them and for the 17 output columns
//   the block           ONE allocation: 25 double columns (the 24 and the loop kernel's scratch column draw_log, photon_cols.hpp), then idx, flags
//                       and type, each on a 256-byte boundary.  The snapshot and every captured frame are byte images of the block, so "the same
//                       list, elsewhere" is the live pointer plus a byte delta (kernels.hip: copy_list_columns, restore_list_columns_lds)
//   windows             list r of a rank pool is the slots [r * rank_stride, r * rank_stride + n) of every column
//   the derived columns and the flag byte of a list that comes in as columns
//   the output block    the records, the 17 compacted output columns, their type column and the scan's scratch (get_output, the outbox)
// Plain C++ (no HIP calls): it compiles with g++ -std=c++17.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mcrat_hip.h"
#include "device_types.hpp"

namespace mcrat {

// ------------------------------------------------------------------ the column tables
constexpr int N_PHOTON_COLS = 24;     // PhotonDev's double columns
constexpr int N_ABI_COLS = 19;        // ... of which the first 19 are the caller's (mcrat_hip_photon_soa); the other five are derived
constexpr int N_BLOCK_COLS = 25;      // the block's double columns: the 24 and draw_log
constexpr int N_OUTPUT_COLS = 17;     // OutputCols::col (launch.hpp)

constexpr double *PhotonDev::*PHOTON_COLS[N_PHOTON_COLS] = {
    &PhotonDev::r0, &PhotonDev::r1, &PhotonDev::r2, &PhotonDev::p0, &PhotonDev::p1, &PhotonDev::p2, &PhotonDev::p3,
    &PhotonDev::c0, &PhotonDev::c1, &PhotonDev::c2, &PhotonDev::c3, &PhotonDev::s0, &PhotonDev::s1, &PhotonDev::s2, &PhotonDev::s3,
    &PhotonDev::num_scatt, &PhotonDev::weight, &PhotonDev::tau, &PhotonDev::tts,
    &PhotonDev::u0, &PhotonDev::u1, &PhotonDev::u2, &PhotonDev::ntau, &PhotonDev::tau_next};
// the caller's member for column k < N_ABI_COLS
constexpr double *mcrat_hip_photon_soa::*SOA_COLS[N_ABI_COLS] = {
    &mcrat_hip_photon_soa::r0, &mcrat_hip_photon_soa::r1, &mcrat_hip_photon_soa::r2,
    &mcrat_hip_photon_soa::p0, &mcrat_hip_photon_soa::p1, &mcrat_hip_photon_soa::p2, &mcrat_hip_photon_soa::p3,
    &mcrat_hip_photon_soa::comv_p0, &mcrat_hip_photon_soa::comv_p1, &mcrat_hip_photon_soa::comv_p2, &mcrat_hip_photon_soa::comv_p3,
    &mcrat_hip_photon_soa::s0, &mcrat_hip_photon_soa::s1, &mcrat_hip_photon_soa::s2, &mcrat_hip_photon_soa::s3,
    &mcrat_hip_photon_soa::num_scatt, &mcrat_hip_photon_soa::weight, &mcrat_hip_photon_soa::total_optical_depth, &mcrat_hip_photon_soa::time_to_scatter};
// the caller's member for output column k, in OutputCols order (staging.hip, output_write_kernel)
constexpr double *mcrat_hip_output_columns::*OUTPUT_COLS[N_OUTPUT_COLS] = {
    &mcrat_hip_output_columns::p0, &mcrat_hip_output_columns::p1, &mcrat_hip_output_columns::p2, &mcrat_hip_output_columns::p3,
    &mcrat_hip_output_columns::comv_p0, &mcrat_hip_output_columns::comv_p1, &mcrat_hip_output_columns::comv_p2, &mcrat_hip_output_columns::comv_p3,
    &mcrat_hip_output_columns::r0, &mcrat_hip_output_columns::r1, &mcrat_hip_output_columns::r2,
    &mcrat_hip_output_columns::s0, &mcrat_hip_output_columns::s1, &mcrat_hip_output_columns::s2, &mcrat_hip_output_columns::s3,
    &mcrat_hip_output_columns::num_scatt, &mcrat_hip_output_columns::weight};

// ------------------------------------------------------------------ the block
inline size_t photon_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct PhotonLayout {
    int n_pad;                        // capacity: max(n, 1) rounded up to a multiple of 2 * STEP_BLOCK
    size_t col[N_BLOCK_COLS];         // byte offsets of the double columns ...
    size_t idx, flags, type;          // ... and of the three others
    unsigned col_stride;              // doubles from one column to the next (= n_pad: 8 * n_pad is a multiple of 256)
    size_t total;                     // bytes
};
enum PhotonLayoutStatus { PHOTON_LAYOUT_OK = 0, PHOTON_LAYOUT_TOO_MANY_SLOTS };      // the loop kernel indexes column k as k * col_stride + slot in 32 bits
inline const char *photon_layout_text(PhotonLayoutStatus s) { return s == PHOTON_LAYOUT_TOO_MANY_SLOTS ? "photon list: more than 2^32 / 25 slots" : ""; }
inline PhotonLayoutStatus photon_layout(int n, PhotonLayout *l)
{
    const size_t n_pad = photon_align_up((size_t)(n > 1 ? n : 1), 2 * STEP_BLOCK);
    if (n_pad * N_BLOCK_COLS > 0xffffffffull) return PHOTON_LAYOUT_TOO_MANY_SLOTS;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = photon_align_up(off + bytes, 256); return o; };
    for (int k = 0; k < N_BLOCK_COLS; ++k) l->col[k] = take(sizeof(double) * n_pad);
    l->idx = take(sizeof(int) * n_pad);
    l->flags = take(n_pad);
    l->type = take(n_pad);
    l->total = off;
    l->n_pad = (int)n_pad;
    l->col_stride = (unsigned)((l->col[1] - l->col[0]) / sizeof(double));
    return PHOTON_LAYOUT_OK;
}

// How the loop kernel reaches slot i of a global column (photon_cols.hpp, ListCols): as the column's wave-uniform base plus the slot's zero-extended
// 32-bit BYTE offset, i * 8, where every slot's offset fits -- n_pad * 8 < 2^32, n_pad the capacity of the block the columns lie in -- and as the
// 32-bit index k * col_stride + i otherwise.  photon_layout's own bound is the tighter one (25 columns against 8 bytes), so every block it lays out has
// byte offsets, and the loop kernels are built with them only: PHOTON_ADDR_INDEX names the accessor they had before, of which no build exists, so a
// launch asks (kernels.hip, launch_rank_loop: the accessor's precondition, checked where the kernel is started) and refuses a block that has none.
enum PhotonAddressing { PHOTON_ADDR_INDEX = 0, PHOTON_ADDR_BYTE_OFFSET = 1 };
constexpr PhotonAddressing photon_addressing(size_t n_pad) { return n_pad * sizeof(double) <= 0xffffffffull ? PHOTON_ADDR_BYTE_OFFSET : PHOTON_ADDR_INDEX; }
static_assert(photon_addressing(0xffffffffull / N_BLOCK_COLS) == PHOTON_ADDR_BYTE_OFFSET, "a block photon_layout accepts has 32-bit byte offsets");

// the block at `base` as the kernels' PhotonDev, for a list of n slots
inline PhotonDev bind_photons(const PhotonLayout &l, void *base, int n)
{
    char *b = static_cast<char *>(base);
    PhotonDev p{};
    for (int k = 0; k < N_PHOTON_COLS; ++k) p.*PHOTON_COLS[k] = reinterpret_cast<double *>(b + l.col[k]);
    p.idx = reinterpret_cast<int *>(b + l.idx);
    p.flags = reinterpret_cast<unsigned char *>(b + l.flags);
    p.type = b + l.type;
    p.n = n;
    p.n_pad = l.n_pad;
    p.col_stride = l.col_stride;
    return p;
}

// list `rank` of a pool as a list of its own: n slots in a window of rank_stride (slots beyond n stay invalid); col_stride stays the pool's -- the
// columns of a view are windows into the pool's
inline PhotonDev photon_window(const PhotonDev &pool, int rank, int rank_stride, int n)
{
    PhotonDev p = pool;
    offset_photons(p, (size_t)rank * (size_t)rank_stride);
    p.n = n;
    p.n_pad = rank_stride;
    return p;
}

// the same block, elsewhere: every pointer moved by byte_delta ...
inline PhotonDev shift_photons(const PhotonDev &ph, long long byte_delta)
{
    PhotonDev p = ph;
    for (int k = 0; k < N_PHOTON_COLS; ++k) p.*PHOTON_COLS[k] = reinterpret_cast<double *>(reinterpret_cast<char *>(ph.*PHOTON_COLS[k]) + byte_delta);
    p.idx = reinterpret_cast<int *>(reinterpret_cast<char *>(ph.idx) + byte_delta);
    p.flags = reinterpret_cast<unsigned char *>(ph.flags) + byte_delta;
    p.type = ph.type + byte_delta;
    return p;
}
// ... where byte_delta takes the live block at live_base to image `index` of the images of block_bytes each that start at image_base (the snapshot:
// index 0; the captures: the frame)
inline long long image_delta(const void *image_base, const void *live_base, long long index, size_t block_bytes)
{
    return (long long)(static_cast<const char *>(image_base) - static_cast<const char *>(live_base)) + index * (long long)block_bytes;
}

// The slots [first, first + n) of a block as copies: `rows` pieces of `width` bytes, `pitch` bytes apart, the first `off` bytes into the block.  The
// 24 columns of PhotonDev as one extent, then idx, flags and type; the scratch column is not among them (the loop kernel writes it before it reads it).
struct CopyExtent { size_t off, pitch, width, rows; };
constexpr int N_WINDOW_EXTENTS = 4;
inline void window_extents(const PhotonLayout &l, size_t first, size_t n, CopyExtent out[N_WINDOW_EXTENTS])
{
    out[0] = CopyExtent{l.col[0] + sizeof(double) * first, sizeof(double) * l.col_stride, sizeof(double) * n, (size_t)N_PHOTON_COLS};
    out[1] = CopyExtent{l.idx + sizeof(int) * first, 0, sizeof(int) * n, 1};
    out[2] = CopyExtent{l.flags + first, 0, n, 1};
    out[3] = CopyExtent{l.type + first, 0, n, 1};
}

// ------------------------------------------------------------------ a list that comes in as columns
inline unsigned char make_flags(char type, double weight, int recalc)
{
    unsigned f = FLAG_VALID;
    if (type != 'p' && weight != 0) f |= FLAG_MOVES;      // mclib.c:1070
    if (recalc == 1) f |= FLAG_RECALC;
    return (unsigned char)f;
}
// the derived columns (device_types.hpp) into out[4 * n] -- u0, u1, u2, ntau, n each: same operations, in the same order, as mclib.c:1074-1080 and
// :680.  A photon with p0 == 0 gets u = 0; without a tau column every -1 / tau is -1 / 0.
inline void derived_columns(int n, const double *p0, const double *p1, const double *p2, const double *p3, const double *tau_or_null, double *out)
{
    const size_t N = (size_t)n;
    for (size_t i = 0; i < N; ++i) {
        double u0 = 0.0, u1 = 0.0, u2 = 0.0;
        if (p0[i] != 0) {
            const double d = 1.0 / p0[i];
            u0 = p1[i] * d * C_LIGHT;
            u1 = p2[i] * d * C_LIGHT;
            u2 = p3[i] * d * C_LIGHT;
        }
        out[i] = u0; out[N + i] = u1; out[2 * N + i] = u2;
        const double tau = tau_or_null ? tau_or_null[i] : 0.0;
        out[3 * N + i] = -1.0 / tau;
    }
}

// ------------------------------------------------------------------ the output block
// What saveCheckpoint and printPhotons read, staged in one buffer: the records of n_records slots (0: none), then -- when the output is wanted -- the 17
// compacted columns of m photons, their type column and the scan's scratch of scan_ints ints (the count per 256 slots -> first output slot).  Every
// piece on a 256-byte boundary; m == 0 keeps room for one photon.  [0, copy_bytes) is what goes to the host: the scan's scratch stays, and so do the
// columns of an output without photons.
struct OutputLayout {
    size_t rec, rec_bytes, col[N_OUTPUT_COLS], type, scan, total, copy_bytes;
};
inline OutputLayout output_layout(size_t m, size_t scan_ints, int n_records, bool want_output = true)
{
    OutputLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = photon_align_up(off + bytes, 256); return o; };
    l.rec = take(sizeof(mcrat_hip_photon) * (size_t)n_records);
    l.rec_bytes = l.copy_bytes = off;
    if (want_output) {
        const size_t room = m ? m : 1;
        for (int k = 0; k < N_OUTPUT_COLS; ++k) l.col[k] = take(sizeof(double) * room);
        l.type = take(room);
        if (m) l.copy_bytes = off;
        l.scan = take(sizeof(int) * scan_ints);
    }
    l.total = off;
    return l;
}
// the block at `base` as the caller's output columns (count is left alone)
inline void bind_output(const OutputLayout &l, void *base, mcrat_hip_output_columns *cols)
{
    char *b = static_cast<char *>(base);
    for (int k = 0; k < N_OUTPUT_COLS; ++k) cols->*OUTPUT_COLS[k] = reinterpret_cast<double *>(b + l.col[k]);
    cols->type = b + l.type;
}

}  // namespace mcrat
