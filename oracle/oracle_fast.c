/*
 * oracle_fast.c -- the engine's FAST mode (MCRAT_HIP_MODE_FAST, mcrat_amd/csrc/kernels.hip "FAST mode") restated on the CPU,
 * sequentially and one photon at a time.   TEST INFRASTRUCTURE ONLY (see mcrat_oracle.h).
 *
 * The reference has no such mode: its loop (mcrat.c:761-851) is driven by the events of the whole list.  Within a frozen hydro frame the
 * photons do not see each other, so the same steps can be taken photon by photon, each on its own clock, with random numbers keyed by
 * (photon, pass) instead of drawn from one stream.  What the reference does to ONE photon in one iteration is kept step for step, through
 * the oracle's own functions:
 *
 *   locate        findContainingHydroCell's loop body (mclib.c:447-604, orc_locatePhoton).  find_nearest_grid_switch is 1 in the first
 *                 iteration of a frame (mcrat.c:756), so pass 0 re-locates a photon that is inside the domain and has a cell whether or not
 *                 it is still in that cell; later passes re-locate it when it has left its cell.  Outside the domain, or without a
 *                 cell: nearest_block_index = -1 (mclib.c:592).
 *   free time     calcMeanFreePath's loop body (mclib.c:657-687): the optical depth is recomputed when recalc_properties is set (after the
 *                 photon's own scattering), the free path is -log(u) / tau with the pass's uniform, 1e12 cm without a cell.
 *   flight        the photon's clocks: t_left, the frame time it still has, and w_left, what is left of the current one of `windows` equal
 *                 time windows.  limit = min(t_left, w_left):
 *                     t < limit          fly t, scatter at the end of the flight (in this pass);
 *                     in the last window fly limit (= t_left): the frame is over for this photon;
 *                     otherwise          fly limit to the window's boundary: t_left -= limit, w_left = window -- the next pass looks at the
 *                                        cell again and draws again, as the reference does for every photon whenever any photon of the
 *                                        list has scattered.
 *                 There are `windows` windows, counted: the last one ends with the frame, i.e. it is as long as the clock says is left.
 *                 (Comparing the two clocks instead -- "the frame is over when t_left <= w_left" -- compares, in the last window, two
 *                 numbers that are equal but for the roundings of the flights subtracted from them: whether a photon then takes one pass
 *                 more, through a sliver of a window some 1e-17 s long and with a draw of its own, would hang on the last bit of a logarithm.)
 *                 A photon without a cell streams t_left and is done.  Positions advance as updatePhotonPosition advances them
 *                 (mclib.c:1054-1100): not for a photon without weight, nor for one of the cyclo-synchrotron pool.
 *   scattering    photonEvent's body for one candidate (mclib.c:1144-1322, orc_scatterCandidate) with the event stream of (pass, slot).  A
 *                 Klein-Nishina rejection leaves the photon as it was; it draws again in the next pass.
 *
 * With windows == 1 and a list of one photon this IS the reference's loop (own clock and list clock are the same clock), which
 * tests/test_oracle_fast.py checks against orc_photon_loop on one tape of uniforms.
 */
#include "mcrat_oracle.h"
#include <float.h>
#include <math.h>
#include <string.h>

static void note_margin(double *m, double value, double scale)
{
    const double d = fabs(value) / scale;
    if (d < *m) *m = d;                                  /* (a NaN never lowers it) */
}

void orc_fast_frame(const orc_config *c, orc_photon_list *l, const orc_hydro *h, orc_rng *rng, double remaining_time, int windows,
                    uint32_t slot_base, orc_fast_counts *cnt, orc_fast_margins *mg, double *flown, int *n_pass)
{
    orc_stats st;
    long long scatterings = 0;
    memset(&st, 0, sizeof st);
    memset(cnt, 0, sizeof *cnt);
    mg->flight = DBL_MAX;
    mg->kn = DBL_MAX;
    if (flown) for (int i = 0; i < l->list_capacity; i++) flown[i] = 0;
    if (n_pass) for (int i = 0; i < l->list_capacity; i++) n_pass[i] = 0;
    if (!(remaining_time > 0) || windows < 1) return;
    const double window = remaining_time / (double)windows;
    orc_kn_margin_watch(&mg->kn);

    for (int i = 0; i < l->list_capacity; i++) {
        orc_photon *ph = &l->photons[i];
        const uint32_t slot = (uint32_t)i + slot_base;
        const int moves = (ph->type != ORC_CS_POOL_PHOTON) && (ph->weight != 0);      /* mclib.c:1070 */
        double t_left = remaining_time, w_left = (windows == 1) ? remaining_time : window, sum = 0;
        long long pass = 0;
        int done = 0, w_index = 0;                                                    /* the window the photon is in: 0 .. windows - 1 */
        while (!done) {
            orc_rng_set_iteration(rng, (uint64_t)pass);

            cnt->relocated += orc_locatePhoton(c, ph, slot, h, pass == 0, &st, rng);

            double mfp;
            if (ph->nearest_block_index != -1) {                                      /* mclib.c:657-681 */
                if (ph->recalc_properties == 1) {
                    orc_calculateOpticalDepth_keyed(c, ph, h, rng, slot);
                    ph->recalc_properties = 0;
                }
                const double rnd = orc_rng_fast_freepath_draw(rng, slot);
                mfp = (-1.0 / ph->total_optical_depth) * log(rnd);
            } else {
                mfp = 1e12;
            }
            const double t = mfp / ORC_C_LIGHT;
            ph->time_to_scatter = t;                                                  /* mclib.c:687 */

            double fly;
            int scatters = 0;
            if (ph->nearest_block_index == -1) {                                      /* out of the frame's cells: streams to the frame's end */
                fly = t_left;
                t_left = 0;
                done = 1;
            } else {
                const double limit = fmin(t_left, w_left);
                note_margin(&mg->flight, t - limit, limit);
                if (t < limit) {
                    fly = t;
                    t_left -= fly;
                    w_left -= fly;
                    scatters = 1;
                } else if (w_index == windows - 1) {
                    fly = t_left;
                    t_left = 0;
                    done = 1;
                } else {
                    fly = limit;
                    t_left -= fly;
                    w_index += 1;
                    w_left = (w_index == windows - 1) ? t_left : window;
                }
            }
            if (moves) {                                                              /* mclib.c:1070-1080 */
                const double divide_p0 = 1.0 / ph->p0;
                ph->r0 += ph->p1 * divide_p0 * ORC_C_LIGHT * fly;
                ph->r1 += ph->p2 * divide_p0 * ORC_C_LIGHT * fly;
                ph->r2 += ph->p3 * divide_p0 * ORC_C_LIGHT * fly;
            }
            sum += fly;
            if (scatters) orc_scatterCandidate(c, ph, slot, h, &scatterings, rng, &st);
            pass += 1;
        }
        cnt->photon_steps += pass;
        if (pass > cnt->passes) cnt->passes = pass;
        if (flown) flown[i] = sum;
        if (n_pass) n_pass[i] = (int)pass;
    }
    orc_kn_margin_watch(NULL);
    cnt->scatterings = scatterings;
    cnt->kn_rejections = st.kn_rejections;
    cnt->not_found = st.not_found;
}
