/*
 * mcrat_hip.h -- C ABI of the MI355X photon-loop engine (libmcrat_hip.so).
 *
 * Drop-in boundary for ONE path of lazzati-astro/MCRaT: the per-timestep photon
 * loop `while (remaining_time > 0)` of Src/mcrat.c:761-851 and the functions it
 * calls (findContainingHydroCell mclib.c:436, calcMeanFreePath mclib.c:617,
 * photonEvent mclib.c:1107, updatePhotonPosition mclib.c:1054) plus the
 * per-frame reductions around it (phMinMax mclib.c:1465, phScattStats
 * mclib.c:1385, averagePhotonEnergy mclib.c:1358).
 *
 * The reference has no plugin/FFI interface: its boundary is the set of C
 * functions main() calls on caller-owned structs (Src/mclib.h:8-29).  This
 * header keeps those structs' layouts (so MCRaT's own photonInjection,
 * saveCheckpoint, printPhotons keep working on the host side) and replaces the
 * loop by frame-granular calls, because a host<->device round trip per scatter
 * event would cost more than the event.  INTEGRATION.md shows the edit to
 * mcrat.c; DESIGN.md the device side.
 *
 * Conventions (mirroring the reference where it has any):
 *   - plain C, plain pointers and sizes; the library never takes ownership of
 *     caller memory and never calls exit(); every entry point returns 0 on
 *     success or a negative MCRAT_HIP_E* code (the caller keeps the reference's
 *     fatal behaviour, e.g. mcrat.c:904-915);
 *   - one context per MPI rank / GPU; a context is not thread safe (the
 *     reference runs one thread per rank);
 *   - the "cell not found" log lines of geometry.c:382 / mclib.c:583 are
 *     reported as counters in mcrat_hip_frame_stats;
 *   - there is NO CPU fallback: if the device or the code object is missing
 *     mcrat_hip_init fails with MCRAT_HIP_ENODEV.
 */
#ifndef MCRAT_HIP_H
#define MCRAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: these declarations are its whole surface */
#endif

#define MCRAT_HIP_ABI_VERSION 1

/* error codes */
#define MCRAT_HIP_OK        0
#define MCRAT_HIP_EINVAL   (-1)  /* bad argument / unsupported switch combination        */
#define MCRAT_HIP_ENODEV   (-2)  /* no usable gfx950 device or code object                */
#define MCRAT_HIP_ENOMEM   (-3)  /* device or host allocation failed                      */
#define MCRAT_HIP_EHIP     (-4)  /* a HIP runtime call failed (see mcrat_hip_last_error)  */
#define MCRAT_HIP_ESTATE   (-5)  /* call out of order (e.g. run before set_hydro)         */
#define MCRAT_HIP_EREFUSED (-6)  /* the reference refuses this too and goes on (rebinCyclosynchCompPhotons' early returns); nothing changed */

/* switch values: identical to Src/mcrat.h:36-44,64-65 so a -D of mcrat_input.h maps 1:1 */
#define MCRAT_HIP_CARTESIAN        0
#define MCRAT_HIP_SPHERICAL        1
#define MCRAT_HIP_CYLINDRICAL      2
#define MCRAT_HIP_POLAR            3
#define MCRAT_HIP_TWO              0
#define MCRAT_HIP_TWO_POINT_FIVE   1
#define MCRAT_HIP_THREE            2
#define MCRAT_HIP_TAU_DIRECT       1
#define MCRAT_HIP_TAU_TABLE        2   /* needs mcrat_hip_set_hot_cross_section before the first frame */

/* the compile-time switches of Src/mcrat_input.h:49-71 that the loop depends on */
typedef struct mcrat_hip_config {
    int abi_version;             /* MCRAT_HIP_ABI_VERSION                                     */
    int dimensions;              /* DIMENSIONS                                                */
    int geometry;                /* GEOMETRY                                                  */
    int stokes_switch;           /* STOKES_SWITCH   (0/1)                                     */
    int tau_calculation;         /* TAU_CALCULATION: MCRAT_HIP_TAU_DIRECT or MCRAT_HIP_TAU_TABLE */
    int cyclosynchrotron_switch; /* CYCLOSYNCHROTRON_SWITCH; 1 needs virtual_rank_photons = 0  */
    int device;                  /* HIP device ordinal                                        */
    void *stream;                /* hipStream_t to launch on, or NULL for a private stream    */
    uint32_t rng_stream;         /* virtual-rank id mixed into every RNG counter (rank id)    */
    int iterations_per_sync;     /* loop iterations queued between host status reads (0: 256) */
    int use_graph;               /* replay the iteration batch as a hipGraph (0/1)            */
    int profile;                 /* bracket every step-kernel launch with HIP events (0/1)    */
    int virtual_rank_photons;    /* 0: the photon list is ONE list with one clock (one MPI rank of the reference).
                                    n > 0: the list is split into ceil(capacity/n) *virtual ranks* of n consecutive
                                    slots, each an independent photon list with its own clock and RNG stream
                                    (rng_stream + r) -- the reference's many-small-ranks run shape
                                    (Doc/mcrat_doc.tex:165-166,222) on one GPU; see DESIGN.md section 2 */
} mcrat_hip_config;

/* == struct photon, Src/mcrat.h:142-171 (thermal-only build): 176 bytes on x86-64,
 * offsets type@0 p0@8 ... num_scatt@128 recalc_properties@136 weight@144
 * nearest_block_index@152 time_to_scatter@160 total_optical_depth@168 */
typedef struct mcrat_hip_photon {
    char   type;
    double p0, p1, p2, p3;
    double comv_p0, comv_p1, comv_p2, comv_p3;
    double r0, r1, r2;
    double s0, s1, s2, s3;
    double num_scatt;
    int    recalc_properties;
    double weight;
    int    nearest_block_index;
    double time_to_scatter;
    double total_optical_depth;
} mcrat_hip_photon;

/* == struct photonList, Src/mcrat.h:173-180 */
typedef struct mcrat_hip_photon_list {
    mcrat_hip_photon *photons;
    int *sorted_indexes;
    int num_photons;
    int num_null_photons;
    int list_capacity;
} mcrat_hip_photon_list;

/* column form of the same record (host pointers, n entries each); any pointer may be
 * NULL on get (column skipped).  On set, NULL comv_p, s, time_to_scatter and
 * total_optical_depth columns mean zeros; the other columns are required. */
typedef struct mcrat_hip_photon_soa {
    int n;
    char   *type;
    double *p0, *p1, *p2, *p3;
    double *comv_p0, *comv_p1, *comv_p2, *comv_p3;
    double *r0, *r1, *r2;
    double *s0, *s1, *s2, *s3;
    double *num_scatt;
    int    *recalc_properties;
    double *weight;
    int    *nearest_block_index;
    double *time_to_scatter;
    double *total_optical_depth;
} mcrat_hip_photon_soa;

/* the members of struct hydro_dataframe (Src/mcrat.h:194-244) the loop reads; host pointers
 * of num_elements doubles.  r2, r2_size, v2 may be NULL in 2-D. */
typedef struct mcrat_hip_hydro {
    int num_elements;
    const double *r0, *r1, *r2;
    const double *r0_size, *r1_size, *r2_size;
    const double *v0, *v1, *v2;
    const double *dens_lab, *temp, *gamma;
    double r0_domain[2], r1_domain[2], r2_domain[2];
    double fps;
} mcrat_hip_hydro;

/* what main() logs after the loop (mcrat.c:810-817,881-892) plus throughput counters */
typedef struct mcrat_hip_frame_stats {
    long long iterations;                    /* passes of the while loop                         */
    long long photon_steps;                  /* iterations x list_capacity                       */
    long long frame_scatt_cnt;               /* mclib.c:1318                                     */
    long long num_photons_find_new_element;  /* mclib.c:579,608-611                              */
    long long not_found;                     /* "Hydro grid index not found" events, mclib.c:583 */
    long long kn_rejections;                 /* candidates that drew an electron but did not scatter */
    long long rescans;                       /* times the candidate list had to be refilled      */
    int    last_scattered_index;             /* *scattered_ph_index, mclib.c:1341                */
    double last_scattered_temp;              /* hydro temp of its cell, mcrat.c:813              */
    double last_time_step;                   /* time_step, mcrat.c:781,844                       */
    double remaining_time;
    double time_now;
    double step_kernel_ms;                   /* profile=1: summed duration of step-kernel launches */
    long long step_kernel_launches;
    double event_kernel_ms;                  /* profile=1: summed duration of event-kernel launches */
    long long table_fallbacks;                  /* TAU_CALCULATION == TABLE: look-ups off the table whose cross section was integrated afresh (mcrat_hip_set_hot_cross_section) */
    long long slot_steps;                    /* slots actually taken through a pass, summed over the passes: = photon_steps, except that a
                                                cyclo-synchrotron list's settled null slots behind its last photon (the half a doubled list consists of,
                                                Src/photons.c:112-121) take no part in a pass here although the reference walks them (Src/mclib.c:620,684) --
                                                the figure a roofline is computed from */
} mcrat_hip_frame_stats;

typedef struct mcrat_hip_ctx mcrat_hip_ctx;

/* lifetime ------------------------------------------------------------------ */
int  mcrat_hip_init(mcrat_hip_ctx **ctx, const mcrat_hip_config *cfg);
void mcrat_hip_destroy(mcrat_hip_ctx *ctx);
const char *mcrat_hip_version(void);
const char *mcrat_hip_strerror(int code);
const char *mcrat_hip_last_error(const mcrat_hip_ctx *ctx);   /* text of the last HIP failure */
/* A context belongs to the device it was created on (mcrat_hip_config.device), and HIP's "current device" is a property of the host thread:
 * a thread other than the creating one calls this once before it uses the context (two pools per GPU with a host thread each: INTEGRATION.md).
 * One context, one thread at a time. */
int mcrat_hip_bind_thread(mcrat_hip_ctx *ctx);

/* staging: once per hydro frame (after getHydroData, mcrat.c:721) ------------- */
int mcrat_hip_set_hydro(mcrat_hip_ctx *ctx, const mcrat_hip_hydro *hydro);

/* getHydroData (mcrat_io.c:1898-1990; mcrat.c:640,721) on the device, file reading excluded: the caller hands over the
 * buffers a reader holds right after its H5Dread / fread calls, in code units; the expansion to cells, the unit
 * scaling, the slab selection with the reader's elem_factor loop, the derived columns (gamma, dens_lab, temp),
 * fillHydroCoordinateToSpherical (geometry.c:156) and the SIMULATION_TYPE overwrite (analytic_outflows.c) run on the
 * device, in the reference's cell order, and the result is staged exactly as mcrat_hip_set_hydro would stage it -- no
 * host copy of the selected frame is made (mcrat_hip_get_hydro returns one when the caller needs it).
 *   mcrat_hip_ingest_flash  replaces readAndDecimate (mclib_flash.c:60-431) after line 197 (datasets read)
 *   mcrat_hip_ingest_pluto  replaces readPluto (mclib_pluto.c:1058-1459) after line 1128 (file read)
 *   mcrat_hip_ingest_chombo replaces readPlutoChombo (mclib_pluto.c:12-801) after its HDF5 reads
 * mcrat_host_read_pluto (mcrat_amd/host) parses grid.out, dbl.out and the .dbl file into mcrat_hip_pluto_grid. */
typedef struct mcrat_hip_slab {           /* the selecting arguments of getHydroData (mcrat_io.h:26) + frame constants */
    double r_inj;
    int    ph_inj_switch;                 /* 1: every cell with r > 0.95 r_inj (injection frame); 0: the photons' slab */
    double min_r, max_r, min_theta, max_theta;   /* phMinMax of the photon list (mcrat.c:716) */
    double fps;                           /* hydro_data->fps */
    double r0_domain[2], r1_domain[2], r2_domain[2];   /* hydro_data->r*_domain (mc.par / mcrat_input.h) */
} mcrat_hip_slab;

typedef struct mcrat_hip_flash_blocks {   /* the datasets of a FLASH checkpoint, mclib_flash.c:143-193 */
    int n_blocks;                         /* dims[0] of "coordinates" */
    int coord_stride, bsize_stride;       /* doubles per row of "coordinates" / "block size" */
    const double *coordinates, *block_size;
    const int    *node_type;              /* leaf blocks have 1 */
    const double *velx, *vely, *dens, *pres;   /* [n_blocks][1][8][8] */
    double l_scale, d_scale, p_scale;     /* HYDRO_L_SCALE, HYDRO_D_SCALE, HYDRO_P_SCALE */
} mcrat_hip_flash_blocks;

typedef struct mcrat_hip_pluto_grid {     /* a PLUTO .dbl frame: readGridFile's arrays + the variable blocks */
    int nx, ny, nz;                       /* nz ignored unless DIMENSIONS == THREE */
    const double *x1, *dx1, *x2, *dx2, *x3, *dx3;   /* cell centres and widths per axis, code units (mclib_pluto.c:951-971) */
    const double *rho, *vx1, *vx2, *vx3, *prs;      /* [nz][ny][nx]; vx3 may be NULL in 2-D */
    double l_scale, d_scale, p_scale;
} mcrat_hip_pluto_grid;

typedef struct mcrat_hip_chombo_level {   /* one "level_<i>" group of a PLUTO-Chombo file, mclib_pluto.c:206-276,349-430 */
    int n_boxes;
    const int *boxes;                     /* "boxes": n_boxes x {lo_i, lo_j, [lo_k], hi_i, hi_j, [hi_k]} (the compound type of :48-58) */
    const int *box_offsets;               /* "data:offsets=0": start of each box's data within the level, in doubles */
    long long data_len;                   /* length of "data:datatype=0" */
    int prob_domain[6];                   /* attribute prob_domain, same member order as a box */
    int ref_ratio, logr;                  /* attributes ref_ratio, logr */
    double dx, dombeg1, dombeg2, dombeg3, g_x2stretch, g_x3stretch;   /* attributes dx, domBeg1-3, g_x2stretch, g_x3stretch */
} mcrat_hip_chombo_level;

typedef struct mcrat_hip_chombo {         /* a PLUTO-Chombo AMR frame after readPlutoChombo's HDF5 reads */
    int num_levels, num_vars;             /* attributes num_levels, num_components */
    const mcrat_hip_chombo_level *levels; /* level 0 (coarsest) first */
    const char *const *var_names;         /* attributes component_0 ... ("rho", "vx1", "vx2", "vx3", "prs", ...) */
    const double *data;                   /* the levels' "data:datatype=0", level 0 first (all_data, :151-155,:360) */
    double l_scale, d_scale, p_scale;
} mcrat_hip_chombo;

#define MCRAT_HIP_SCIENCE                       0   /* SIMULATION_TYPE, mcrat.h:30-33 */
#define MCRAT_HIP_CYLINDRICAL_OUTFLOW           1
#define MCRAT_HIP_SPHERICAL_OUTFLOW             2
#define MCRAT_HIP_STRUCTURED_SPHERICAL_OUTFLOW  3
typedef struct mcrat_hip_outflow {        /* the constants analytic_outflows.c hard-codes (lines 5, 65, 140-141) */
    int simulation_type;
    double gamma_infinity;                /* gamma_0 of the structured fireball */
    double lumi, r00;
    double t_comov, ddensity;             /* cylindrical outflow */
    double theta_j, p;                    /* structured fireball */
} mcrat_hip_outflow;
void mcrat_hip_outflow_defaults(int simulation_type, mcrat_hip_outflow *out);   /* the reference's values */

typedef struct mcrat_hip_ingest_result {
    int num_elements;                     /* hydro_data->num_elements */
    int elem_factor;                      /* the reader's log line "Elem factor: %d" */
    long long cells_read;                 /* cells examined (leaf blocks x 64, or nx ny nz) */
} mcrat_hip_ingest_result;

/* outflow may be NULL (SCIENCE).  MCRAT_HIP_EINVAL with last_error set when no elem_factor up to 1000 selects a cell
 * (the reference would loop forever). */
int mcrat_hip_ingest_flash(mcrat_hip_ctx *ctx, const mcrat_hip_flash_blocks *blocks, const mcrat_hip_slab *slab,
                           const mcrat_hip_outflow *outflow, mcrat_hip_ingest_result *result);
int mcrat_hip_ingest_pluto(mcrat_hip_ctx *ctx, const mcrat_hip_pluto_grid *grid, const mcrat_hip_slab *slab,
                           const mcrat_hip_outflow *outflow, mcrat_hip_ingest_result *result);

/* replaces readPlutoChombo (mclib_pluto.c:12-801) after line 430 (levels read).  Cells are numbered level by level, box
 * by box, x fastest, as the reader numbers them; coarse cells covered by a finer level are dropped exactly where the
 * reference drops them -- in injection frames (ph_inj_switch != 0, :672,:745) and not in the photons'-slab branch
 * (:659,:703), which does not consult good_node_buffer.  The per-level 1-D coordinate arrays (:446-517, with libm's exp
 * for logarithmic radial grids) are computed on the host; boxes must lie inside their level's prob_domain and their
 * data must follow one another in "data:offsets=0" order. */
int mcrat_hip_ingest_chombo(mcrat_hip_ctx *ctx, const mcrat_hip_chombo *frame, const mcrat_hip_slab *slab,
                            const mcrat_hip_outflow *outflow, mcrat_hip_ingest_result *result);

/* every column of the staged frame (struct hydro_dataframe, mcrat.h:194-244), host pointers of num_elements doubles
 * allocated by the caller; NULL pointers are skipped.  After mcrat_hip_set_hydro the columns that call did not carry
 * (dens, pres) read as zero. */
typedef struct mcrat_hip_hydro_columns {
    int num_elements;                     /* in: capacity of the arrays; out: elements written */
    double *r0, *r1, *r2, *r0_size, *r1_size, *r2_size;
    double *v0, *v1, *v2;
    double *dens, *dens_lab, *pres, *temp, *gamma;
    double *r, *theta;
} mcrat_hip_hydro_columns;
int mcrat_hip_get_hydro(mcrat_hip_ctx *ctx, mcrat_hip_hydro_columns *out);

/* The consumers after a frame: what printPhotons and saveCheckpoint read from the photon list.
 *   mcrat_hip_get_output         printPhotons' gathering loop (mcrat_io.c:137-181): the photons with weight != 0, in slot
 *                                order, as the arrays it hands to H5Dwrite (datasets P0-3, COMV_P0-3, R0-2, S0-3, NS, PW, PT),
 *                                compacted on the device.  count: in, capacity of the arrays; out, photons written.  With
 *                                every pointer NULL the call only reports the count (MCRAT_HIP_EINVAL + the needed count if
 *                                the capacity is too small).  NULL columns are skipped (COMV_SWITCH / STOKES_SWITCH / SAVE_TYPE
 *                                OFF builds).  The reference holds these arrays on the stack (mcrat_io.c:123-124).
 *   mcrat_hip_get_photons_range  struct photon records of the slots first .. first+count-1 (saveCheckpoint's fwrite loop,
 *                                mcrat_io.c:883-896, in pieces: a 10^8-photon list is 17.6 GB as records).  Bytes between
 *                                the members are zero. */
typedef struct mcrat_hip_output_columns {
    int count;
    double *p0, *p1, *p2, *p3;
    double *comv_p0, *comv_p1, *comv_p2, *comv_p3;
    double *r0, *r1, *r2;
    double *s0, *s1, *s2, *s3;
    double *num_scatt, *weight;
    char   *type;
} mcrat_hip_output_columns;
int mcrat_hip_get_output(mcrat_hip_ctx *ctx, mcrat_hip_output_columns *out);
/* saveCheckpoint's in-place type conversion in CYCLOSYNCHROTRON_SWITCH builds (mcrat_io.c:896-900, :951-955, :991-995), on the resident
 * list: every comptonised photon 'k' with weight != 0 becomes an unabsorbed one 'c' -- before the records are streamed out, and for
 * good, so that the next frame's phAbsCyclosynch (mc_cyclosynch.c:1607) and printPhotons' PT see what the reference's would.
 * mcrat_host_save_checkpoint calls it when its cyclosynchrotron_switch argument is on.  *num_converted may be NULL. */
int mcrat_hip_convert_comptonized(mcrat_hip_ctx *ctx, int *num_converted);
int mcrat_hip_get_photons_range(mcrat_hip_ctx *ctx, int first, int count, mcrat_hip_photon *records);

/* The same two consumers WHILE THE NEXT FRAME RUNS.  The reference calls saveCheckpoint (mcrat.c:902; mcrat_io.c:838-1009) and printPhotons
 * (mcrat.c:907; mcrat_io.c:114-836) at the end of every frame with the rank idle; an outbox takes what they read off the device without
 * holding the loop up:
 *   mcrat_hip_outbox_post   stages the records of ALL slots (want_records) and/or the compacted output columns (want_output; what
 *                           mcrat_hip_get_output returns) in device memory of the outbox, in the context's stream order, and starts their copy
 *                           into pinned host memory on a stream of the outbox's own.  When it returns the photons may change: begin the next
 *                           frame.  Posting again waits for the previous post's copy.
 *   mcrat_hip_outbox_wait   blocks until the copy has landed; may be called from another thread (a writer).  The pointers address the outbox's
 *                           pinned memory and stay valid until the next post on the same outbox (columns: all 17 + type; count photons).
 * Two outboxes give a double buffer: frame f written from one while frame f+1 is posted into the other (mcrat_host_run_ranks does this). */
typedef struct mcrat_hip_outbox mcrat_hip_outbox;
int  mcrat_hip_outbox_create(mcrat_hip_ctx *ctx, mcrat_hip_outbox **box);
void mcrat_hip_outbox_destroy(mcrat_hip_outbox *box);
int  mcrat_hip_outbox_post(mcrat_hip_ctx *ctx, mcrat_hip_outbox *box, int want_records, int want_output);
int  mcrat_hip_outbox_wait(mcrat_hip_outbox *box, const mcrat_hip_photon **records, int *n_records, mcrat_hip_output_columns *cols);

/* Cyclo-synchrotron: the stages of a scatter frame with CYCLOSYNCHROTRON_SWITCH on.  They work on whatever photon
 * types the list holds; mcrat_hip_scatter_frame_cyclosynch (below) chains them as mcrat.c:706-878 does and needs a context created
 * with cyclosynchrotron_switch = 1.
 *   mcrat_hip_set_hydro_extras   the columns of struct hydro_dataframe the magnetic field needs and mcrat_hip_hydro does not carry:
 *                                dens (comoving density; B_FIELD_CALC INTERNAL_E / TOTAL_E, mc_cyclosynch.c:82-83) and B0-2
 *                                (B_FIELD_CALC == SIMULATION).  NULL pointers are skipped; after mcrat_hip_ingest_* dens is there already.
 *   mcrat_hip_absorb_cyclosynch  phAbsCyclosynch (mc_cyclosynch.c:1571-1623): every photon with weight != 0 and a cell whose comoving
 *                                frequency is at or below its cell's cyclotron frequency, and every pool photon, becomes a null
 *                                slot (setNullPhoton, photons.c:210-250); returns the count, the number of comptonised / unabsorbed
 *                                photons left (:1610-1614) and the weight of the absorbed 'i' / 'c' photons (the return value). */
typedef struct mcrat_hip_cyclosynch {
    int    b_field_calc;                  /* B_FIELD_CALC: 0 INTERNAL_E, 1 TOTAL_E, 2 SIMULATION (mcrat.h:47-49) */
    double epsilon_b;                     /* EPSILON_B */
    double rebin_e_perc, rebin_ang, rebin_ang_phi;   /* CYCLOSYNCHROTRON_REBIN_* (mcrat.h:310-321); unused by the absorption */
    int    scatt_frame_number, inj_frame_number;     /* hydro_data->scatt_frame_number / ->inj_frame_number; unused by the absorption */
} mcrat_hip_cyclosynch;
int mcrat_hip_set_hydro_extras(mcrat_hip_ctx *ctx, const double *dens, const double *B0, const double *B1, const double *B2);
/*   mcrat_hip_emit_cyclosynch_pool  photonEmitCyclosynch with inject_single_switch == 0 (mc_cyclosynch.c:1200-1460, mcrat.c:741) on the staged
 *                                frame: pool photons (type 'p') at the centres of the cells of the shell the injected photons occupy
 *                                (calcCyclosynchRLimits with cs->scatt_frame_number / inj_frame_number), each at its cell's cyclotron
 *                                frequency, the common weight adjusted until 1 <= N <= rebin_e_perc * maximum_photons; they go into
 *                                the list's null slots in slot order, the list doubling first when it has none (addToPhotonList,
 *                                photons.c:108-208; MCRAT_HIP_EINVAL where the reference exits with "Adding to the photon list has
 *                                failed").  The Poisson mean is gsl_integration_qags of the Planck photon density from 10 Hz to the
 *                                cyclotron frequency (:1276): QUADPACK's first 21-point rule, which is where QAGS stops while the
 *                                cyclotron frequency lies in the Rayleigh-Jeans tail (every cell of a GRB jet); a cell whose rule
 *                                does not meet QAGS' first-step test is integrated by bisection of the interval with the largest
 *                                error estimate, as the oracle does (oracle_cyclosynch.c, orc_qags: no epsilon extrapolation), with at
 *                                most 64 intervals.  *integrals_not_converged counts the cells that ran out of intervals; if there are
 *                                any the call returns MCRAT_HIP_EREFUSED and emits nothing. */
int mcrat_hip_emit_cyclosynch_pool(mcrat_hip_ctx *ctx, const mcrat_hip_cyclosynch *cs, double r_inj, double ph_weight, int maximum_photons,
                                   double theta_min, double theta_max, double fps, uint64_t seed, int *num_emitted, double *ph_weight_adjusted,
                                   int *integrals_not_converged);
/*   mcrat_hip_rebin_cyclosynch   rebinCyclosynchCompPhotons (mc_cyclosynch.c:246-712): every photon that is neither null, pool nor injected is
 *                                replaced by one 'k' photon per non-empty (log10 energy, polar angle of the position[, azimuth]) bin with the
 *                                bin's weight and weighted averages (bins filled in slot order, so the sums are the reference's sums);
 *                                returns the number of empty bins in *empty_bins and the two counters the reference updates
 *                                (:689-690).  MCRAT_HIP_EREFUSED on the reference's own refusals, which leave the list as it was: nothing to
 *                                rebin, more bins than max_photons, zero bins along an axis, a photon outside the histograms, too few null
 *                                slots (MCRAT_HIP_EINVAL is a bad argument). */
int mcrat_hip_rebin_cyclosynch(mcrat_hip_ctx *ctx, const mcrat_hip_cyclosynch *cs, int max_photons, int *empty_bins, int *num_cyclosynch_ph_emit,
                               int *scatt_cyclosynch_num_ph);
/*   mcrat_hip_scatter_frame_cyclosynch   the scatter-frame body of main() with CYCLOSYNCHROTRON_SWITCH on (mcrat.c:706-878, from the pool emission
 *                                to the absorption; the hydro frame is staged and the extras set): emit_pool is the condition
 *                                `(scatt_frame != scatt_framestart) || (restrt == CONTINUE)` of :707,:727,:855; inside the loop a pool
 *                                photon that photonEvent reports becomes a comptonised one and is replaced by a new pool photon of its
 *                                weight in its cell (:786-795; photonEmitCyclosynch with inject_single_switch = 1, the list doubling
 *                                when it has no null slot), and every 1000 scatterings the comptonised photons are rebinned once there
 *                                are more than max_photons of them (:797-808).  Needs a context created with
 *                                cyclosynchrotron_switch = 1 (one list per context -- many lists: mcrat_hip_pool_scatter_frames_cyclosynch --, no shared clock; mcrat_hip_run
 *                                and mcrat_hip_propagate_frame refuse such a context).  max_iterations <= 0: until the frame is over. */
typedef struct mcrat_hip_cyclosynch_counts {
    int    num_cyclosynch_ph_emit, scatt_cyclosynch_num_ph, frame_abs_cnt;   /* the counters of mcrat.c:735-878.  scatt_cyclosynch_num_ph is IN/OUT:
                                             main() carries it from one scatter frame of an injection to the next (set at mcrat.c:873, reset at
                                             :921) -- pass the previous frame's value in (0 for the first frame; zero the struct before use) */
    int    rebins;                        /* successful rebinCyclosynchCompPhotons calls */
    int    integrals_not_converged;       /* see mcrat_hip_emit_cyclosynch_pool */
    int    pad;
    double n_comptonized;                 /* mcrat.c:788,871 */
    double pool_weight;                   /* ph_weight_adjusted of the pool emission */
} mcrat_hip_cyclosynch_counts;
int mcrat_hip_scatter_frame_cyclosynch(mcrat_hip_ctx *ctx, const mcrat_hip_cyclosynch *cs, double *time_now, double remaining_time, uint64_t seed,
                                       double r_inj, double ph_weight_suggest, int max_photons, double theta_min, double theta_max, double fps,
                                       int emit_pool, long long max_iterations, mcrat_hip_frame_stats *stats, mcrat_hip_cyclosynch_counts *counts);
int mcrat_hip_num_photon_slots(const mcrat_hip_ctx *ctx);   /* photon_list->list_capacity as the device holds it (it grows when the pool does not fit) */
int mcrat_hip_absorb_cyclosynch(mcrat_hip_ctx *ctx, const mcrat_hip_cyclosynch *cs, int *num_abs_ph, int *scatt_cyclosynch_num_ph,
                                double *abs_weight);

/* photonInjection (mclib.c:9-300; mcrat.c:645) on the device, from the staged hydro frame: afterwards the context holds
 * the new photons (*num_photons of them, all of weight *ph_weight_adjusted -- the reference's min/max-photons loop of
 * mclib.c:87-136 runs on the device counts) exactly as if they had been injected on the host and handed to
 * mcrat_hip_set_photons; mcrat_hip_get_photons returns them as struct photon records (the caller allocates
 * *num_photons of them, as setPhotonList would).  spect: 'b' black body, 'w' Wien (mc.par); fps as in hydro_dataframe.
 * The random numbers are the engine's keyed source with the reference's draw order (seed: any 64-bit value, e.g. the
 * gsl_rng_get() of the rank); the Poisson counts come from the engine's own sampler. */
int mcrat_hip_inject_photons(mcrat_hip_ctx *ctx, double r_inj, double ph_weight, int min_photons, int max_photons, char spect,
                             double theta_min, double theta_max, double fps, uint64_t seed, int *num_photons, double *ph_weight_adjusted);

/* TAU_CALCULATION == TABLE, once per run (after initalizeHotCrossSection, hot_x_section.c:29-80): the table
 * getThermalCrossSection interpolates (optical_depth.c:132-149).  thermal_table is the reference's global
 * thermal_table[N_PH_E + 1][N_T + 1] (hot_x_section.c; log10 of the cross section over sigma_T, photon-energy index
 * first), the four bounds are LOG_PH_E_MIN/MAX and LOG_T_MIN/MAX of hot_x_section.h:2-10.  Creating the table
 * (createHotCrossSection, GSL Monte-Carlo integration) stays host-side work of MCRaT; mcrat_host_read_hot_cross_section
 * (mcrat_amd/host) reads the file MCRaT writes.  A lookup outside the table gets what the reference's fallback returns where that is closed-form
 * (interpolateThermalHotCrossSection -> calculateTotalThermalCrossSection, hot_x_section.c:563-599,324-356): below LOG_T_MIN -- every cell colder
 * than 5.9e5 K with the reference's bounds -- the Klein-Nishina cross section of the photon's comoving energy, or 1 when that is below LOG_PH_E_MIN
 * too (:337-340).  The remaining cases (a photon energy beyond the table at a tabulated temperature, or a temperature above LOG_T_MAX) are the
 * reference's Monte-Carlo integral of the cross section at that (energy, temperature) -- calculateTotalThermalCrossSection's 500 000 samples, here
 * from the keyed source: the integral of (pass, slot) has its own 256 substreams, so its value does not depend on which kernel or how many lanes
 * compute it (one wavefront per look-up in the rank pool's loop: milliseconds; one lane in list, shared-clock and FAST mode: a fifth of a second --
 * like the reference, which reports every such look-up on stderr, the loop treats them as rare).  mcrat_hip_frame_stats.table_fallbacks counts them. */
int mcrat_hip_set_hot_cross_section(mcrat_hip_ctx *ctx, const double *thermal_table, int n_ph_e, int n_t,
                                    double log_ph_e_min, double log_ph_e_max, double log_t_min, double log_t_max);

/* `calls` of that integral (hot_x_section.c:348: 500 000, the default); calls <= 0 only asks.  Returns the value in force (a pool's lists follow
 * their pool).  For tests, and for runs that would rather take a coarser integral than wait. */
int mcrat_hip_table_fallback_calls(mcrat_hip_ctx *ctx, int calls);

/* createHotCrossSection (hot_x_section.c:82-133) on the device: fills thermal_table[(n_ph_e + 1) * (n_t + 1)] (photon-energy
 * index first, log10 of the cross section over sigma_T) with the Monte-Carlo integrals of calculateTotalThermalCrossSection
 * (:324-357; `calls` samples per entry, 500 000 in the reference) over the Maxwell-Juttner electrons of
 * singleMaxwellJuttner (electron.c:538) and boostedCrossSection (:370-400).  The samples come from the engine's keyed random
 * source (the reference's are its GSL generator's: the table agrees within the Monte-Carlo error, ~1e-3), entry by entry
 * independent of the launch shape.  The table is returned to the host -- write it with mcrat_host_write_hot_cross_section
 * for later runs, hand it to mcrat_hip_set_hot_cross_section for this one.  221 x 81 entries x 500 000 samples: under a
 * second (a quarter of an hour on one host core). */
int mcrat_hip_create_hot_cross_section(mcrat_hip_ctx *ctx, double *thermal_table, int n_ph_e, int n_t, double log_ph_e_min,
                                       double log_ph_e_max, double log_t_min, double log_t_max, long long calls, uint64_t seed);

/* photons host -> device (after photonInjection mcrat.c:645 / readCheckpoint) and back
 * (before saveCheckpoint mcrat.c:902 / printPhotons mcrat.c:907).  NULL-photon slots
 * (type 'N', weight 0, index -1: photons.c:208) are carried through unchanged.  list_capacity must equal
 * mcrat_hip_num_photon_slots on get; a context with cyclosynchrotron_switch on also sets num_photons and num_null_photons
 * from what the list holds now (photons.c:252-275). */
int mcrat_hip_set_photons(mcrat_hip_ctx *ctx, const mcrat_hip_photon_list *list);
/* Optional, once per allocation (after allocatePhotonListMemory, photons.c:28 / reallocatePhotonListMemory): page-lock the caller's
 * array so that set_photons / get_photons move it by direct DMA at the link's rate -- pageable memory goes through the runtime's
 * staging buffers at a third of that.  Unregister before free()/realloc(). */
int mcrat_hip_register_host(mcrat_hip_ctx *ctx, void *ptr, size_t bytes);
int mcrat_hip_unregister_host(mcrat_hip_ctx *ctx, void *ptr);
int mcrat_hip_get_photons(mcrat_hip_ctx *ctx, mcrat_hip_photon_list *list);
int mcrat_hip_set_photons_soa(mcrat_hip_ctx *ctx, const mcrat_hip_photon_soa *soa);
int mcrat_hip_get_photons_soa(mcrat_hip_ctx *ctx, const mcrat_hip_photon_soa *soa);
int mcrat_hip_num_photon_slots(const mcrat_hip_ctx *ctx);

/* Several contexts on one GPU that are in the same hydro frame -- rank pools on their own HIP streams with a host thread each (INTEGRATION.md,
 * "Two pools per GPU") -- need one copy of the staged frame, its per-cell records, its lookup grid and the cross-section table, not one each:
 * after this call `ctx` reads `owner`'s.  The owner must keep that frame (no re-staging, no mcrat_hip_destroy) while others read it; staging a
 * frame on `ctx` itself (mcrat_hip_set_hydro, mcrat_hip_ingest_*) or sharing again ends the arrangement.  Same DIMENSIONS / GEOMETRY /
 * TAU_CALCULATION and device on both. */
int mcrat_hip_share_hydro(mcrat_hip_ctx *ctx, mcrat_hip_ctx *owner);

/* the loop -------------------------------------------------------------------- */
/* replaces mcrat.c:754-851 for one hydro frame: sets find_nearest_grid_switch=1,
 * runs until remaining_time is used up, updates *time_now, fills *stats.
 * `seed` is the per-frame seed; the reference draws one at mcrat.c:701
 * (gsl_rng_set(rng, gsl_rng_get(rng))) -- pass that gsl_rng_get value. */
int mcrat_hip_propagate_frame(mcrat_hip_ctx *ctx, double *time_now, double remaining_time,
                              uint64_t seed, mcrat_hip_frame_stats *stats);

/* SURVEY.md 8(b)'s `mode` argument.  MCRAT_HIP_MODE_EXACT is mcrat_hip_propagate_frame: the event-driven loop of mcrat.c:761-851,
 * one scattering per pass per list, comparable pass by pass with the reference.  MCRAT_HIP_MODE_FAST runs every photon through the
 * frame on its own clock with per-photon keyed random numbers (photons are independent within a frozen frame and exponential free
 * paths are memoryless): statistically equivalent, NOT sequence-equivalent -- spectra, scattering counts and polarisation agree with
 * the exact mode within Monte-Carlo error (tests/test_gpu_fast_mode.py), single photons do not.  fast_windows is how often
 * per frame a photon's cell and optical depth are refreshed besides after its own scatterings; the reference refreshes them whenever
 * any photon of the rank scatters, i.e. -- for its ranks of about 1000 photons -- as often as the frame has scatterings per 1000 photons.
 * fast_windows <= 0 follows that: the scatterings per 1000 photons of the LIST's previous FAST frame (a pool's list: kept on its view, so that a
 * list's photons do not depend on which other lists share the pool; mcrat_hip_fast_cadence reads and sets it -- a driver that restarts a run hands
 * the value back, or the restarted list begins at 32 again), between 8 and 2048 (32 for the
 * first frame); a fixed 8 is biased by about a per cent in frames with tens of scatterings per photon.  Works on a single list, virtual ranks or a rank pool alike (the lists do not matter to it);
 * refuses cyclo-synchrotron contexts and an attached shared clock.  stats: iterations = passes of the longest-running workgroup,
 * photon_steps = free-path draws, frame_scatt_cnt, kn_rejections, num_photons_find_new_element, not_found. */
#define MCRAT_HIP_MODE_EXACT 0
#define MCRAT_HIP_MODE_FAST  1
int mcrat_hip_propagate_frame_mode(mcrat_hip_ctx *ctx, double *time_now, double remaining_time, uint64_t seed, int mode, int fast_windows,
                                   mcrat_hip_frame_stats *stats);
/* FAST mode for the lists of a rank pool in one launch ([n_ranks] arrays, as mcrat_hip_pool_begin_frames): list r with open[r] != 0 runs its
 * frame of remaining_time[r] with its own seed, stream and list-local slot numbers in its keys -- exactly what
 * mcrat_hip_propagate_frame_mode(view r, ..., seeds[r], MCRAT_HIP_MODE_FAST, ...) gives, so a list's photons do not depend on which other
 * lists share the pool; stats[r]: the list's counters, time_now[r] + remaining_time[r].  mcrat_hip_propagate_frame_mode(pool, FAST) is this
 * for every list that holds photons with one seed and one frame time. */
int mcrat_hip_pool_propagate_frames_fast(mcrat_hip_ctx *pool, const int *open, const uint64_t *seeds, const double *time_now,
                                         const double *remaining_time, int fast_windows, mcrat_hip_frame_stats *stats);
/* the learnt refresh cadence of a list (a context holding one list, or a view of a pool): returns it; set_windows > 0 sets it first (clamped to 8..2048) */
int mcrat_hip_fast_cadence(mcrat_hip_ctx *ctx, int set_windows);

/* the same loop in pieces, for bounded runs (benchmarks, tests, progress logging):
 * begin_frame resets the per-frame state; each run executes at most max_iterations
 * passes (<= 0: until the frame time is used up) and is synchronous on return. */
int mcrat_hip_begin_frame(mcrat_hip_ctx *ctx, uint64_t seed, double time_now, double remaining_time);
int mcrat_hip_run(mcrat_hip_ctx *ctx, long long max_iterations, mcrat_hip_frame_stats *stats);

/* keep / bring back a device-side copy of the resident photons (repeatable frames without a host round trip) */
int mcrat_hip_snapshot_photons(mcrat_hip_ctx *ctx);
int mcrat_hip_restore_photons(mcrat_hip_ctx *ctx);

/* virtual-rank mode: number of lists, and the loop statistics / clock of one of them */
int mcrat_hip_num_virtual_ranks(const mcrat_hip_ctx *ctx);
int mcrat_hip_rank_stats(mcrat_hip_ctx *ctx, int rank, mcrat_hip_frame_stats *stats);

/* Rank pool: the reference's run shape on one GPU ------------------------------------------------------------------
 * MCRaT is run as 150-600 MPI ranks of 10^3 - 5*10^3 photons (Doc/mcrat_doc.tex:165-166,222): every rank owns an
 * (angle bin, injection-frame range) of mcrat.c:139-164,457-479, a Poisson-sized photon list (mclib.c:87-136), its own
 * generator (mcrat.c:99-103,701), its own clock, and its own mc_proc_<rank>.h5 / mc_chkpt_<rank>.dat
 * (mcrat_io.c:199-200,871-903); ranks never talk inside the loop.  A pool lets ONE process per GPU adopt R such ranks:
 *   mcrat_hip_pool_create   turns `pool` into R lists of up to slots_per_rank slots each (slots_per_rank >= the longest list
 *                           a rank will ever hold: max_photons, times the doublings cyclo-synchrotron emission may need)
 *   mcrat_hip_pool_rank     the *view* of list `rank`: a context whose photons, loop state and clock are that list's and
 *                           whose hydro frame is the pool's.  Every per-list entry point of this header works on a view
 *                           exactly as on a context of its own holding only that list with rng_stream `rng_stream`:
 *                           mcrat_hip_set_photons / _inject_photons (the rank joins), _begin_frame (its seed and clock),
 *                           _ph_minmax, _scatt_stats, _get_output, _get_photons_range, _get_photons ... A view is
 *                           destroyed with mcrat_hip_destroy or with its pool; set_hydro / ingest go to the pool.
 *   mcrat_hip_run(pool)     the loop of mcrat.c:761-851 for every list whose view has an open frame (mcrat_hip_begin_frame
 *                           on the view), all lists in ONE launch, one workgroup per list (rank_loop_kernel) -- each list
 *                           sees exactly the arithmetic and the random numbers of a context of its own.  The stats are the
 *                           totals; mcrat_hip_frame_statistics(view) gives a list's own.  mcrat_hip_begin_frame(pool)
 *                           opens a frame for all lists at once with one seed and clock.
 *   mcrat_hip_pool_summaries  phMinMax, phScattStats, averagePhotonEnergy and printPhotons' photon count for every list in
 *                           one launch (lists that do not exist: list_capacity 0 and every other member 0).  With the pool's
 *                           cyclosynchrotron_switch on, max_scatt, min_scatt, avg_scatt, avg_r and avg_energy are over the photons
 *                           with weight != 0 only, as mcrat_hip_scatt_stats and mcrat_hip_avg_energy say below; min_r .. max_theta,
 *                           num_output and list_capacity do not depend on the switch.
 * mcrat_host_run_ranks (mcrat_amd/host) is main()'s rank logic on top of this; INTEGRATION.md shows the edit. */
typedef struct mcrat_hip_rank_summary {
    double min_r, max_r, min_theta, max_theta;   /* phMinMax, mclib.c:1465 */
    double avg_scatt, avg_r;                     /* phScattStats, mclib.c:1385; switch on: photons with weight != 0 only (:1401) */
    double avg_energy;                           /* averagePhotonEnergy, mclib.c:1358; switch on: the same filter (:1373) */
    int    max_scatt, min_scatt;                 /* phScattStats; switch on and no weighted photon: 0 and INT_MAX */
    int    num_output;                           /* photons with weight != 0: what printPhotons writes (mcrat_io.c:137-181) */
    int    list_capacity;                        /* photon_list->list_capacity of this rank (0: no list) */
} mcrat_hip_rank_summary;
/* mcrat_hip_config.profile = 1: the summed duration (HIP events on the context's stream) and the number of the loop kernel's launches since
 * the context was created -- mcrat_hip_run's and mcrat_hip_pool_scatter_frames_cyclosynch's (there: rank_loop_kernel with the hook inside;
 * emission, rebinning and absorption are NOT in it).  MCRAT_HIP_ESTATE without profile. */
int mcrat_hip_profile_totals(const mcrat_hip_ctx *ctx, double *loop_kernel_ms, long long *loop_kernel_launches);
int mcrat_hip_pool_create(mcrat_hip_ctx *pool, int n_ranks, int slots_per_rank);
int mcrat_hip_pool_rank(mcrat_hip_ctx *pool, int rank, uint32_t rng_stream, mcrat_hip_ctx **view);
int mcrat_hip_pool_summaries(mcrat_hip_ctx *pool, mcrat_hip_rank_summary *out /* [n_ranks] */);
/* the same for hundreds of lists at once, so that a frame of the pool costs a handful of launches, not a handful per list:
 *   mcrat_hip_pool_begin_frames  mcrat_hip_begin_frame for every list with open[r] != 0, each with its own seed and clock ([n_ranks] arrays)
 *   mcrat_hip_pool_frame_stats   mcrat_hip_frame_statistics of every list ([n_ranks]; lists without a frame: what they last had)
 *   mcrat_hip_pool_layout        the lists' places in the pool's own slot numbering: list r occupies the slots r * slots_per_rank ...,
 *                                which mcrat_hip_get_photons_range / mcrat_hip_get_output on the POOL context address (slots beyond a
 *                                list's length hold no photon: type 0, weight 0) -- one transfer for all lists' records or columns */
/* CYCLOSYNCHROTRON_SWITCH on (the pool created from a context with cyclosynchrotron_switch = 1): mcrat_hip_scatter_frame_cyclosynch for
 * every list with lists[r].open != 0 -- pool emission per list, then the loops of ALL lists in the same launches (a list leaves the loop only
 * for the hook of mcrat.c:786-808: its scattered pool photon converted and replaced, the list doubling inside its window of the pool when
 * it has no null slot left, the rebinning trigger), rebinning and absorption at the end.  cs carries the build's switches (b_field_calc,
 * epsilon_b, rebin_*); the frame numbers come per list.  slots_per_rank of mcrat_hip_pool_create must allow for the doublings
 * (MCRAT_HIP_ENOMEM otherwise).  stats / counts: [n_ranks], per list; stats may be NULL. */
typedef struct mcrat_hip_pool_cs_list {
    int      open;
    int      emit_pool;                   /* (scatt_frame != scatt_framestart) || (restrt == CONTINUE), mcrat.c:707 */
    int      scatt_frame_number, inj_frame_number;
    uint64_t seed;
    double   time_now, remaining_time;
    double   r_inj, ph_weight_suggest, theta_min, theta_max;
} mcrat_hip_pool_cs_list;
int mcrat_hip_pool_scatter_frames_cyclosynch(mcrat_hip_ctx *pool, const mcrat_hip_cyclosynch *cs, int max_photons, double fps,
                                             const mcrat_hip_pool_cs_list *lists, mcrat_hip_frame_stats *stats, mcrat_hip_cyclosynch_counts *counts);
/* photonInjection (mcrat_hip_inject_photons) for every list of the pool with inject != 0, a handful of launches for all of them: each list gets
 * exactly the photons mcrat_hip_inject_photons(view, ...) would give it (same keys, same order); num_photons / ph_weight_adjusted are filled.
 * lists: [n_ranks]; the lists' views must exist (mcrat_hip_pool_rank). */
typedef struct mcrat_hip_pool_inject_list {
    int      inject;
    char     spect;                        /* 'b' or 'w' */
    int      min_photons, max_photons;
    double   r_inj, ph_weight, theta_min, theta_max;
    uint64_t seed;
    int      num_photons;                  /* out */
    double   ph_weight_adjusted;           /* out */
    int      status;                       /* out: MCRAT_HIP_OK, or why THIS list was not injected (the other lists are; the call returns the first
                                            *      such code).  Arguments are validated for all lists before any window is touched. */
} mcrat_hip_pool_inject_list;
int mcrat_hip_pool_inject_photons(mcrat_hip_ctx *pool, double fps, mcrat_hip_pool_inject_list *lists);
/* mcrat_hip_set_photons for `count` lists of the pool at once -- a CONTINUE run's restart, every adopted rank's checkpointed list (readCheckpoint,
 * Src/mcrat_io.c:1011): the records cross PCIe in one copy and reach their windows in one launch.  rank_of[j]: the pool rank of lists[j] (its view
 * exists, no rank twice).  Each list ends up exactly as mcrat_hip_set_photons(view, &lists[j]) leaves it; everything is validated first. */
int mcrat_hip_pool_set_photons(mcrat_hip_ctx *pool, int count, const int *rank_of, const mcrat_hip_photon_list *lists);
int mcrat_hip_pool_begin_frames(mcrat_hip_ctx *pool, const int *open, const uint64_t *seeds, const double *time_now, const double *remaining_time);
int mcrat_hip_pool_frame_stats(mcrat_hip_ctx *pool, mcrat_hip_frame_stats *out /* [n_ranks] */);
int mcrat_hip_pool_layout(const mcrat_hip_ctx *pool, int *n_ranks, int *slots_per_rank);
/* The frame queue: every list of the pool through SEVERAL hydro frames in ONE launch.  The reference's ranks are asynchronous processes, each in its
 * own frame loop (Src/mcrat.c:457-479, :566-934: nothing makes rank A wait for rank B at the end of a hydro frame); one launch per hydro frame does,
 * and a third of such a launch is the tail of its last lists.  Here the loop kernel's workgroups are persistent and take
 * (frame, list) items in frame-major order: a list that is through frame f starts f + 1 while others are still in f.  Every list runs exactly the
 * frames mcrat_hip_pool_begin_frames + mcrat_hip_run would have given it one at a time -- the same seeds, clocks, passes, photons, bit for bit.
 * All arrays are [n_frames * n_ranks], frame-major (item f * n_ranks + r); a list's open frames must be consecutive (a rank joins at its injection
 * frame and stays, mcrat.c:566-700).  chain_clock: a list's clock carries over from its previous frame of the call -- time_now = where that frame ended,
 * remaining_time = frame_end - time_now (mcrat.c:757 with frame_end = (scatt_frame + increment_scatt_frame) / fps) -- and time_now / remaining_time
 * are used for its first frame only; else every frame takes its own time_now and remaining_time.  restore_each_frame: every frame starts from
 * the lists as mcrat_hip_snapshot_photons saved them (benchmarks: the same work every frame).  hydro: NULL, or [n_frames] contexts holding the
 * staged hydro frame of frame f (mcrat_hip_set_hydro / mcrat_hip_ingest_* on them, same device and switches as the pool; NULL entry: the pool's own
 * frame; the contexts keep their frames staged while the call runs) -- a real run stages frame f + 1 for the slab the photons can reach from frame
 * f (phMinMax widened by c / fps) before the launch: a list in frame f + 1 then finds its photons in the cells of THAT frame, exactly as after
 * mcrat_hip_share_hydro(pool, hydro[f + 1]) + one launch per frame.  stats: [n_frames * n_ranks], what
 * mcrat_hip_pool_frame_stats would have reported after each frame (lists that sat a frame out: zeros); stats[0] also carries the whole call's totals:
 * step_kernel_ms and step_kernel_launches (a context created with profile = 1) and, with TAU_CALCULATION == TABLE, table_fallbacks -- summed over the
 * counters of the pool and of every context named in hydro (each frame's look-ups count on the context its frame is staged on; the call clears them all
 * first).  A list that opens a frame with remaining_time <= 0 runs no pass in it but is still restored (restore_each_frame) and captured
 * (capture_frames) as in any other frame.  Not with the cyclo-synchrotron switch (its hook needs the host between passes).  Afterwards the pool is
 * as after the last frame's mcrat_hip_run. */
typedef struct mcrat_hip_frame_plan {
    int n_frames;
    int chain_clock;
    int restore_each_frame;
    int capture_frames;                   /* 1: the lists as every frame but the last leaves them are kept for mcrat_hip_pool_select_frame */
    const int      *open;
    const uint64_t *seeds;
    const double   *time_now;
    const double   *remaining_time;
    const double   *frame_end;            /* chain_clock only */
    mcrat_hip_ctx *const *hydro;          /* NULL: every frame through the pool's own staged frame */
} mcrat_hip_frame_plan;
int mcrat_hip_pool_run_frames(mcrat_hip_ctx *pool, const mcrat_hip_frame_plan *plan, mcrat_hip_frame_stats *stats /* [n_frames * n_ranks] */);

/* The outputs of the frames of a plan (phScattStats, saveCheckpoint, printPhotons: mcrat.c:881-915 need every list as ITS frame left it, and in a
 * queue launch a list is moved on by its next frame at once).  With plan.capture_frames = 1 each list is copied aside at the end of every frame but
 * the last (the lists that were open in it -- every other slot of a capture reads as an empty one, weight 0; one copy of the pool per such frame in HBM); mcrat_hip_pool_select_frame(pool, f) then makes the pool's
 * read entry points -- mcrat_hip_pool_summaries, mcrat_hip_outbox_post, mcrat_hip_get_photons_range, mcrat_hip_get_output -- look at frame f's copy,
 * until mcrat_hip_pool_select_frame(pool, -1) (the live lists = the last frame).  While a frame is selected mcrat_hip_run and
 * mcrat_hip_pool_run_frames refuse.  The captures are valid until the next mcrat_hip_pool_run_frames. */
int mcrat_hip_pool_select_frame(mcrat_hip_ctx *pool, int frame);

/* function-granular A/B entry points (one kernel each, for parity tests against the
 * reference functions): the findContainingHydroCell + calcMeanFreePath half of an
 * iteration and the photonEvent half.  mcrat_amd/host/mcrat_hip_host.h wraps them in shims with the reference's
 * own signatures (mclib.h:8-29) for A/B runs function by function. */
int mcrat_hip_step_locate_sample(mcrat_hip_ctx *ctx, int find_nearest_block_switch);
int mcrat_hip_frame_statistics(mcrat_hip_ctx *ctx, mcrat_hip_frame_stats *stats);   /* the loop counters so far (synchronises) */
int mcrat_hip_update_photon_position(mcrat_hip_ctx *ctx, double t);   /* updatePhotonPosition, mclib.c:1054-1100, on the resident photons */
int mcrat_hip_step_event(mcrat_hip_ctx *ctx, mcrat_hip_frame_stats *stats);

/* ONE photon list split over several GPUs, ONE clock ------------------------------------------------------------
 * The reference never does this: its ranks own disjoint photons AND disjoint clocks (mcrat.c:761-851 runs per rank;
 * SURVEY.md 8e).  This mode keeps the event order of a single list -- what one rank holding all the photons would
 * compute -- while the N-wide work is spread over `world` GPUs: every GPU owns the contiguous global slots
 * [slot_base, slot_base + n), with n the capacity of its own mcrat_hip_set_photons list.  A round is
 *
 *     mcrat_hip_shared_clock_propose(ctx);          findContainingHydroCell + calcMeanFreePath on the own slots, then
 *                                                    the own earliest candidates (the argsort prefix of mclib.c:702-712)
 *                                                    with the photon data photonEvent needs -> send buffer
 *     all-gather send -> recv over the GPUs          the min-reduction of SURVEY.md 8e; bytes_per_rank each; the host's
 *                                                    job: ncclAllGather / MPI_Allgather on the context's stream
 *     mcrat_hip_shared_clock_resolve(ctx);          photonEvent (mclib.c:1107) on the merged candidates, identically on
 *                                                    every GPU; the owner of the scattered photon stores it
 *
 * and mcrat_hip_shared_clock_poll tells when the frame is over (rounds after that are no-ops, so polling every few
 * dozen rounds is enough).  All contexts of the group use the same rng_stream, seed, time_now and remaining_time;
 * the photons end up bit-identical to a single context holding the concatenated list.  In this mode
 * last_scattered_index in the stats is a GLOBAL slot, num_photons_find_new_element / not_found count the own slots,
 * and `rescans` counts the rounds that continued an undecided iteration.
 * send/recv: device buffers of bytes_per_rank and world * bytes_per_rank bytes; pass NULL to let the library
 * allocate them (read them back with mcrat_hip_shared_clock_buffers); with world == 1 recv may equal send. */
size_t mcrat_hip_shared_clock_bytes_per_rank(void);
int mcrat_hip_shared_clock_attach(mcrat_hip_ctx *ctx, int world, int rank, long long slot_base, void *send, void *recv);
int mcrat_hip_shared_clock_buffers(mcrat_hip_ctx *ctx, void **send, void **recv);
/* The exchange done by the GPUs themselves (one-shot peer writes and a local wait instead of a collective launched by the host):
 *   mcrat_hip_shared_clock_attach_device   attach as above with library-owned, fine-grained (peer-coherent) buffers: a receive buffer of
 *                                          2 x world proposals (the rounds alternate between its halves) and world stamps;
 *   mcrat_hip_shared_clock_peer_buffers    their addresses and sizes, for the caller to hand to the other ranks (hipIpcGetMemHandle between
 *                                          processes, the pointers themselves between contexts of one process or with peer access enabled);
 *   mcrat_hip_shared_clock_set_peers       [world] arrays with every rank's receive buffer and stamps as THIS process addresses them (the own
 *                                          entries are ignored);
 *   mcrat_hip_shared_clock_exchange        between propose and resolve: a kernel writes this rank's proposal into every peer's buffer and
 *                                          stamps it (_push), a second one waits for the stamps of all ranks (_wait; bounded: a peer that
 *                                          never arrives makes the next poll fail with MCRAT_HIP_EHIP instead of hanging the GPU).  A wait
 *                                          that gives up copies nothing and parks the loop: the photons stay at the last pass every rank
 *                                          completed, and the rounds still queued (a captured batch) return at once instead of each
 *                                          spinning its own budget;
 *   mcrat_hip_shared_clock_reset_exchange  after such a failure: clears this rank's give-up word, round number and stamps.  Every rank calls
 *                                          it, then the ranks synchronise (any barrier), then begin_frame as usual.
 * Since round 3 the push runs at the end of the propose kernel and the wait at the head of the resolve kernel (two launches less per round); the
 * three exchange calls then only check the state and return, so a host loop written as propose / exchange / resolve stays as it is.  The peers
 * must therefore be set before the first propose.  MCRAT_HIP_SC_FOLD=0 (environment, read at attach) keeps push and wait as kernels of their own.
 * All on the context's stream and without per-round arguments (the round number lives on the device, the wait kernel copies the round's
 * proposals to the fixed place resolve reads), so propose / exchange / resolve capture into a hipGraph like the collective.  Every rank must run the same
 * number of rounds (rounds after the frame's end are no-ops but still exchange), as with the all-gather. */
int mcrat_hip_shared_clock_attach_device(mcrat_hip_ctx *ctx, int world, int rank, long long slot_base);
int mcrat_hip_shared_clock_peer_buffers(mcrat_hip_ctx *ctx, void **recv, size_t *recv_bytes, void **flags, size_t *flags_bytes);
int mcrat_hip_shared_clock_set_peers(mcrat_hip_ctx *ctx, void *const *peer_recv, void *const *peer_flags);
int mcrat_hip_shared_clock_exchange_push(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_exchange_wait(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_exchange(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_reset_exchange(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_propose(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_resolve(mcrat_hip_ctx *ctx);
int mcrat_hip_shared_clock_poll(mcrat_hip_ctx *ctx, int *frame_done, mcrat_hip_frame_stats *stats);   /* synchronises the stream */
int mcrat_hip_shared_clock_finish(mcrat_hip_ctx *ctx, mcrat_hip_frame_stats *stats);   /* apply the pending advance, final stats */

/* The random stream as an INPUT ("tape").  MCRaT draws everything from one sequential gsl_rng_ranlxs0 stream
 * (Src/mcrat.c:99-103, reseeded per frame :701).  The engine's default source is its own keyed generator (every comparison in tests/ uses it on both
 * sides); with a tape the caller supplies the stream instead -- the doubles MCRaT's generator returned (gsl_rng_type::get_double, in [0,1)), recorded
 * in call order by tools/ref_harness from the UNMODIFIED reference -- and the loop consumes it exactly as MCRaT does:
 *   per pass, one gsl_rng_uniform_pos for every slot with a cell (nearest_block_index != -1), in ascending slot order   (Src/mclib.c:646-675)
 *   then photonEvent's draws for each candidate it tries, in its call order                       (Src/electron.c:81,196,217-233; Src/mcrat_scattering.c:519-574)
 * gsl_rng_uniform_pos skips zeros, gsl_ran_gaussian (polar method) takes as many pairs as it needs: as GSL publishes them.  The photons after a frame
 * can then be held against MCRaT's own, photon for photon ("Pinning parity with your GSL").  STATUS: the tape path is validated against
 * this repository's CPU restatement of MCRaT only (tests/test_gpu_tape.py: engine == oracle on the same tape, zeros on the tape included) -- no tape
 * recorded from MCRaT itself exists yet (the reference needs GSL, which the development image lacks; tools/ref_harness has not been compiled
 * against it).  The product build's arithmetic differs from the reference's IEEE sequence in the last place or two (reciprocals and roots by
 * v_rcp / v_rsq + Newton steps, physics.hpp), so a comparison decided within a few ulp can fall the other way than MCRaT's; a maintainer who wants
 * correctly rounded operands under every decision builds the kernels with -DMCRAT_IEEE_ARITH=1 (slower; physics.hpp).  A validation mode: one list per context
 * (refused on rank pools, virtual ranks, the shared clock and with the cyclo-synchrotron switch), the free-path draws of a pass taken by one
 * workgroup.  uniforms == NULL or n == 0 returns to the keyed source.  While a tape is set the seed of begin_frame / propagate_frame is ignored and
 * the tape is read on across frames (MCRaT's reseeding is part of the recorded stream).
 *   mcrat_hip_rng_tape_position   entries read so far; *ran_out != 0 if the loop needed more than the tape holds (results then meaningless). */
int mcrat_hip_set_rng_tape(mcrat_hip_ctx *ctx, const double *uniforms, long long n);
int mcrat_hip_rng_tape_position(mcrat_hip_ctx *ctx, long long *position, int *ran_out);

/* Tapes for the lists of a rank pool.  MCRaT is run as many MPI ranks, each with its own gsl_rng_ranlxs0 stream (Src/mcrat.c:99-103, reseeded per
 * frame :701); a maintainer who records several ranks replays them here as the lists of one pool.  Per list k: uniforms[k][0, n[k]) are the doubles
 * that rank's generator returned, consumed as mcrat_hip_set_rng_tape consumes them -- per pass one gsl_rng_uniform_pos per located slot in ascending
 * slot order (Src/mclib.c:646-675), then photonEvent's draws (Src/electron.c:81,196,217-233; Src/mcrat_scattering.c:519-574).  uniforms[k] == NULL or
 * n[k] == 0: list k keeps its keyed streams (bit for bit what it gives in a pool without tapes).  Replaces every list's tape; positions start at 0 and
 * carry over from frame to frame.  Every value must lie in [0, 1) (MCRAT_HIP_EINVAL).  A taped list ignores its seed in mcrat_hip_pool_begin_frames
 * and in a frame plan.
 * A pool that holds tapes runs every frame through the tape build of the loop kernel: 256 threads per list, columns in HBM/L2 -- neither the choice
 * of workgroup size nor the MCRAT_HIP_RANK_* overrides apply -- and mcrat_hip_pool_run_frames runs its plan one launch per frame (captures and
 * mcrat_hip_pool_select_frame as there).  Refused with MCRAT_HIP_ESTATE: these calls on a view or a context that is no pool; on a pool that holds tapes,
 * mcrat_hip_pool_propagate_frames_fast, mcrat_hip_pool_scatter_frames_cyclosynch and mcrat_hip_run on one of its views; tapes on a pool with the
 * cyclo-synchrotron switch.  Not covered: mcrat_host_run_ranks (its injection and per-frame reseeding draw from keyed streams).
 *   mcrat_hip_pool_rng_tape_positions   per list: entries read so far (0 for a keyed list), ran_out != 0 if it needed more than its tape holds
 *                                       (that list's results are then meaningless).  Synchronises the stream. */
int mcrat_hip_pool_set_rng_tapes(mcrat_hip_ctx *pool, const double *const *uniforms /* [n_ranks] */, const long long *n /* [n_ranks] */);
int mcrat_hip_pool_rng_tape_positions(mcrat_hip_ctx *pool, long long *position /* [n_ranks] */, int *ran_out /* [n_ranks] */);

/* The device functions of the path, one at a time, on arrays -- for function-level parity tests against the reference functions
 * (tests/test_gpu_functions.py; the loop does not use this entry).  in / out: n rows of doubles, row layouts:
 *   KN_CROSS_SECTION       in  energy_ratio                          out sigma / sigma_T        kleinNishinaCrossSection, mcrat_scattering.c:597
 *   LORENTZ_BOOST_PHOTON   in  beta[3], p[4]                         out p'[4]                  lorentzBoost(.., 'p'), mclib.c:302 (zeroNorm'ed)
 *   LORENTZ_BOOST_ELECTRON in  beta[3], p[4]                         out p'[4]                  lorentzBoost(.., 'e')
 *   STOKES_ROTATION        in  v[3], v_ph[3], v_ph_boosted[3], s[4]  out s[4]                   stokesRotation, mcrat_scattering.c:103
 *   THERMAL_ELECTRON       in  temp, ph[4]                           out el[4]                  singleThermalElectron, electron.c:70
 *   THERMAL_ELECTRON_WAVE  the same through the wavefront-wide sampler the event walk uses (one wavefront per row)
 *   ELECTRON_AND_SCATTER   in  temp, ph[4], s[4]                     out el[4], ph'[4], s'[4], occurred    singleThermalElectron then
 *                                                                    singleScatter (mcrat_scattering.c:151) on one stream; STOKES as the context's
 * The arithmetic forms the loop kernels use instead (physics.hpp, device_types.hpp; tests/test_gpu_loop_arithmetic.py compares them with
 * extended precision).  Every entry calls the function the loop calls:
 *   RCP_NR, RSQRT_NR, SQRT_NR   in  x                                 out 1/x, 1/sqrt(x), sqrt(x)   hardware estimate + two Newton steps
 *   CELL_OPERANDS          in  a, b, c, gamma_cell, dens_lab         out w, nsig, gam, kf, kf_of_gamma(gam)   cell_staged_operands as the
 *                                                                    device staging calls it; (a, b, c) the cell's velocity record
 *   BOOST_WITH_PHOTON      in  b[3], g, kf, p[4]                     out p'[4]                  boost_with<true>: g, kf as given, zero_norm_lean'ed
 *   BOOST_WITH_ELECTRON    in  b[3], g, kf, p[4]                     out p'[4]                  boost_with<false>
 *   BOOST_STAGED_PHOTON    in  b[3], p[4]                            out p'[4]                  boost_with<true> with gam of cell_staged_operands(b)
 *                                                                    and kf_of_gamma(gam): what a re-location runs
 *   OPTICAL_DEPTH_STAGED   in  beta[3] (Cartesian), gamma_cell, dens_lab, p[3], norm   out tau, ntau    optical_depth_staged on the operands of
 *                                                                    cell_staged_operands(beta, gamma_cell, dens_lab); ntau = -rcp_nr(tau)
 *   AZIMUTH                in  x, y                                  out c, s, c_h, s_h         cos_sin_of_atan2(y, x); cos_sin_with_hypot(y, x, h)
 *                                                                    with h = sqrt(x*x + y*y) as hydro_coords hands it over
 *   HYDRO_COORDS           in  x, y, z                               out a0, a1, a2             hydro_coords<DIMENSIONS, geometry> of the context
 *                                                                    (mcratCoordinateToHydroCoordinate, geometry.c:15; -1 where an axis is absent)
 *   THERMAL_CROSS_SECTION  in  photon_comv_e, fluid_temp             out norm, fallback, eps, theta   thermal_cross_section_lookup on the context's
 *                                                                    table: fallback = 1 where the loop would integrate afresh at (eps, theta),
 *                                                                    else 0, 0, 0; norm = 1, 0, 0, 0 on a context without a table (DIRECT).
 *                                                                    MCRAT_HIP_EINVAL while mcrat_hip_create_hot_cross_section runs on the context
 *                                                                    in another thread (a courtesy: a context stays one thread at a time)
 *   KN_CROSS_SECTION_IEEE  in  energy_ratio                          out sigma / sigma_T        kn_cross_section_ieee (the reference's divisions)
 * Random numbers of row i: the engine's event stream {seed, iteration i, slot 0, the context's rng_stream} (rng.hpp).
 * fn outside [1, MCRAT_HIP_FN_COUNT): MCRAT_HIP_EINVAL. */
#define MCRAT_HIP_FN_KN_CROSS_SECTION       1
#define MCRAT_HIP_FN_LORENTZ_BOOST_PHOTON   2
#define MCRAT_HIP_FN_LORENTZ_BOOST_ELECTRON 3
#define MCRAT_HIP_FN_STOKES_ROTATION        4
#define MCRAT_HIP_FN_THERMAL_ELECTRON       5
#define MCRAT_HIP_FN_THERMAL_ELECTRON_WAVE  6
#define MCRAT_HIP_FN_ELECTRON_AND_SCATTER   7
#define MCRAT_HIP_FN_RCP_NR                 8
#define MCRAT_HIP_FN_RSQRT_NR               9
#define MCRAT_HIP_FN_SQRT_NR               10
#define MCRAT_HIP_FN_CELL_OPERANDS         11
#define MCRAT_HIP_FN_BOOST_WITH_PHOTON     12
#define MCRAT_HIP_FN_BOOST_WITH_ELECTRON   13
#define MCRAT_HIP_FN_BOOST_STAGED_PHOTON   14
#define MCRAT_HIP_FN_OPTICAL_DEPTH_STAGED  15
#define MCRAT_HIP_FN_AZIMUTH               16
#define MCRAT_HIP_FN_HYDRO_COORDS          17
#define MCRAT_HIP_FN_THERMAL_CROSS_SECTION 18
#define MCRAT_HIP_FN_KN_CROSS_SECTION_IEEE 19
#define MCRAT_HIP_FN_COUNT                 20   /* one past the last code */
int mcrat_hip_eval_function(mcrat_hip_ctx *ctx, int fn, int n, const double *in, double *out, uint64_t seed);

/* per-frame reductions on the resident photons -------------------------------
 * They follow mcrat_hip_config.cyclosynchrotron_switch as the reference's follow CYCLOSYNCHROTRON_SWITCH (a view: its pool's switch):
 *   mcrat_hip_ph_minmax    photons with weight != 0 only, under either setting (mclib.c:1479); none: (DBL_MAX, 0, DBL_MAX, 0)
 *   mcrat_hip_scatt_stats  switch off: every slot of the list; on: photons with weight != 0 only (mclib.c:1401-1403), so null slots
 *                          and absorbed photons take no part in the extremes, the sums or the count -- none left: max_scatt = 0,
 *                          min_scatt = INT_MAX, both averages NaN (0/0), as in the reference
 *   mcrat_hip_avg_energy   the same rule for both of its sums (mclib.c:1373-1375); none left: NaN
 * (phScattStats' per-type "Avg r for i type ..." log line is not computed.) */
int mcrat_hip_ph_minmax(mcrat_hip_ctx *ctx, double *min_r, double *max_r, double *min_theta, double *max_theta); /* mclib.c:1465 */
int mcrat_hip_scatt_stats(mcrat_hip_ctx *ctx, int *max_scatt, int *min_scatt, double *avg_scatt, double *avg_r); /* mclib.c:1385 */
int mcrat_hip_avg_energy(mcrat_hip_ctx *ctx, double *erg);                                                    /* mclib.c:1358 */

/* mock observations on the resident photons: light curves, spectra, polarisation ---
 * The photons binned by observer, detection time and energy in one pass on the device, without the HDF5 round trip.  The polar axis is r2 / p3.
 * A slot counts when it is part of a list, weight != 0 and its type is neither 'p' (pool photon) nor 'N' (null photon).  Observer o accepts a
 * photon when  p3 <= p0 * cos_lo[o] && p3 > p0 * cos_hi[o]  (its cone as two cosines, cos_lo > cos_hi; cones may overlap, and a photon counts for
 * every observer that accepts it).  Its energy is  e = p0 * C_LIGHT  [erg] and its detection time
 *     t_det = time_now - ((r2 * cos_obs[o] + sqrt(r0 * r0 + r1 * r1) * sin_obs[o]) / C_LIGHT)   [s].
 * Bin k of an axis holds  edges[k] <= x < edges[k + 1]; an accepted photon outside either range is in no bin and counted in n_outside[o].  Per
 * (observer, time bin, energy bin): count, W = sum w, WE = sum w * e, and the Stokes sums I, Q, U, V = sum w * s0 .. s3 (zero with stokes_switch
 * off).  Light curves, spectra, polarisation degree and angle are sums and quotients of these planes: the caller's.
 * Every expression above is evaluated in exactly that order in IEEE double without contraction, so the counts are exact: the same as the same
 * expressions in host code.  The sums are added with floating-point atomics and are NOT bit-reproducible from run to run; each is within
 * (m + 2) * 2^-53 * sum|term| of the exact sum of its bin's m terms.
 * MCRAT_HIP_EINVAL, with its own text in mcrat_hip_last_error: n_obs, n_t or n_e < 1; n_obs * n_t * n_e overflowing an int; cos_lo <= cos_hi;
 * edges that are not finite or not strictly ascending; more edges and observers than the kernel can stage (about 10 000 values together).
 *   mcrat_hip_observe         one list: a stand-alone context, or a view of a pool (that list alone); time_now is the list's clock.
 *   mcrat_hip_pool_observe    every list of a pool in one launch, each with its own clock time_now[r]; reads what mcrat_hip_pool_summaries reads:
 *                             the pool's live columns as they stand, every slot with its valid flag (slots beyond a list's length and lists
 *                             never created carry none).  Like mcrat_hip_pool_summaries it flushes nothing a view holds pending: lists whose
 *                             frames the pool has run (mcrat_hip_run on the pool, mcrat_hip_pool_run_frames) are current; a list stepped one
 *                             by one through its view (mcrat_hip_step_locate_sample, mcrat_hip_step_event) must be observed through that view, which flushes it first.
 *   mcrat_hip_observe_path    how the context's last observation was accumulated: 1 a copy of the cube per workgroup in LDS, flushed once; 2
 *                             atomics straight into the cube in HBM (a cube too large for LDS); 0 none yet.  MCRAT_HIP_OBSERVE_PATH=lds|global
 *                             in the environment forces one (lds is refused for a cube that does not fit).
 * Both calls synchronise before they return. */
typedef struct mcrat_hip_observer {      /* inputs, host pointers */
    int n_obs; const double *cos_obs, *sin_obs, *cos_lo, *cos_hi;   /* [n_obs] */
    int n_t;   const double *t_edges;                               /* [n_t + 1] seconds */
    int n_e;   const double *e_edges;                               /* [n_e + 1] erg */
} mcrat_hip_observer;
typedef struct mcrat_hip_observation {   /* outputs, host pointers, each [n_obs * n_t * n_e], observer-major then time then energy; any may be NULL */
    long long *count; double *w, *we, *i, *q, *u, *v;
    long long *n_accepted, *n_outside;   /* [n_obs] */
} mcrat_hip_observation;
int mcrat_hip_observe(mcrat_hip_ctx *ctx, const mcrat_hip_observer *obs, double time_now, mcrat_hip_observation *out);
int mcrat_hip_pool_observe(mcrat_hip_ctx *pool, const mcrat_hip_observer *obs, const double *time_now /* [n_ranks] */, mcrat_hip_observation *out);
int mcrat_hip_observe_path(const mcrat_hip_ctx *ctx);

/* line-of-sight optical depths and photospheres ---------------------------------
 * A sightline is the straight ray from x_0 = (r0, r1, r2) along the unit vector of a photon 4-momentum (p0, p1, p2, p3) through ONE frozen staged
 * hydro frame; the fluid is piecewise constant per cell and sampled at step midpoints:
 *     ipn = 1 / sqrt((p1*p1 + p2*p2) + p3*p3);   n = (p1*ipn, p2*ipn, p3*ipn);   tau = 0;  path = 0;  k = 0
 *     loop:  if k == max_steps                                    -> status STEP_CAP, stop
 *            rho = sqrt((x*x + y*y) + z*z);  h = step_frac * rho;  if (!(h > h_min)) h = h_min
 *            m = (x + (0.5*h)*n_x, y + (0.5*h)*n_y, z + (0.5*h)*n_z)
 *            m outside the domain (the loop's strict test) or in no cell   -> status LEFT_MESH, stop
 *            kappa [1/cm]: the optical depth per cm of the photon in the lowest-index cell that holds m, the cell's velocity taken at the azimuth
 *                   of m, as the loop computes it; TAU_CALCULATION == TABLE: with the thermal cross section looked up at the photon's comoving
 *                   energy in that cell and the cell's temperature -- where the reference would integrate afresh (off the table at a covered or
 *                   higher temperature)                           -> status OFF_TABLE, stop (no integral is taken here)
 *            tau += kappa*h;  path += h;  x += h*n_x;  y += h*n_y;  z += h*n_z;  k += 1
 *            if tau >= tau_stop                                   -> status OPAQUE, stop          (tau_stop = +inf: never)
 * Per ray: tau, path, steps (= k) and status -- 0 SKIPPED, 1 LEFT_MESH, 2 OPAQUE, 3 STEP_CAP, 4 OFF_TABLE; n_status counts the rays per status.
 * Every position expression is evaluated in exactly this order in IEEE double, with correctly rounded division and square root and without
 * contraction: steps, path and every decision that does not hang on tau are the same as the same expressions in host code.  A kappa that is not
 * a number (a cell at rest: 0/0, as in the reference's cosine) goes into tau as it is.
 * Surface (surface_level >= 0; negative: off): a ray with status LEFT_MESH has the total T = tau and the partial sums S_k (tau after k counted
 * steps, S_0 = 0); surface_step is the smallest k with (T - S_k) <= surface_level and surface_r0 .. r2 is x_k -- the point from which at most
 * surface_level of optical depth is left to the edge of the frame: the photosphere for level 1.  surface_step == 0: the start is already outside
 * the surface.  Every other ray -- another status, the surface off, a T that is not a number -- gets surface_step = -1 and NaN positions.
 *   mcrat_hip_sightline_rays           the caller's n rays (host arrays).
 *   mcrat_hip_sightline_photons        the resident photons of one list (a stand-alone context, or a view of a pool): outputs of
 *                                      mcrat_hip_num_photon_slots entries.  A slot is marched when it is part of the list, weight != 0 and its type
 *                                      is neither 'p' nor 'N' (as the mock observations count it), from its r0 .. r2 along its p0 .. p3; every other
 *                                      slot gets status SKIPPED, tau = path = 0, steps = 0.  A pending advance is flushed first; no column changes.
 *   mcrat_hip_pool_sightline_photons   every slot of a pool in one launch: mcrat_hip_num_photon_slots(pool) entries, list r from r * the pool's
 *                                      slots per list on.  It reads what mcrat_hip_pool_observe reads.
 * hydro: the context whose staged frame the rays cross; NULL: ctx's own.  In a run the staged frame is only the photons' slab, which a ray leaves
 * at once: a caller who wants the optical depth to the edge of the simulation stages the whole frame on a second context and passes it.  It must
 * be on the same device with the same DIMENSIONS, GEOMETRY and TAU_CALCULATION (MCRAT_HIP_EINVAL otherwise).
 * MCRAT_HIP_EINVAL, with its own text in mcrat_hip_last_error, checked in this order: n <= 0; step_frac negative or not finite; h_min not finite or
 * <= 0; max_steps outside 1 .. 1048576; tau_stop NaN or <= 0; surface_level NaN or +inf.  MCRAT_HIP_ESTATE: no staged frame; no photons (the photon
 * forms); TABLE without a cross-section table.  MCRAT_HIP_SIGHTLINE_REFILL=0|1 in the environment picks how rays are dealt to the kernel's lanes
 * (1: a lane whose ray has ended takes the next unclaimed one); the outputs do not depend on it.  Every call synchronises before it returns. */
#define MCRAT_HIP_SIGHTLINE_SKIPPED 0
#define MCRAT_HIP_SIGHTLINE_LEFT_MESH 1
#define MCRAT_HIP_SIGHTLINE_OPAQUE 2
#define MCRAT_HIP_SIGHTLINE_STEP_CAP 3
#define MCRAT_HIP_SIGHTLINE_OFF_TABLE 4
typedef struct mcrat_hip_sightline_params { double step_frac, h_min; int max_steps; double tau_stop, surface_level; } mcrat_hip_sightline_params;
typedef struct mcrat_hip_sightlines {       /* host pointers, [n]; any may be NULL */
    double *tau, *path; int *steps, *status; int *surface_step; double *surface_r0, *surface_r1, *surface_r2;
    long long n_status[5];
} mcrat_hip_sightlines;
int mcrat_hip_sightline_rays(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro /* or NULL */, const mcrat_hip_sightline_params *params, int n,
                             const double *r0, const double *r1, const double *r2, const double *p0, const double *p1, const double *p2,
                             const double *p3 /* host arrays [n] */, mcrat_hip_sightlines *out);
int mcrat_hip_sightline_photons(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, mcrat_hip_sightlines *out);
int mcrat_hip_pool_sightline_photons(mcrat_hip_ctx *pool, const mcrat_hip_ctx *hydro, const mcrat_hip_sightline_params *params, mcrat_hip_sightlines *out);

/* the radiation field on the hydro mesh: per-cell and per-shell photon moments ---
 * The resident photons located in ONE staged hydro frame and summed where they are, in one pass on the device, without the HDF5 round trip.  A slot
 * counts when it is part of a list, weight != 0 and its type is neither 'p' nor 'N' (as the mock observations count it).  For a counted photon, in
 * exactly this order, in IEEE double with correctly rounded division and square root and without contraction:
 *     r = sqrt((r0*r0 + r1*r1) + r2*r2);   mu = r2 / r
 *     (a0, a1, a2) = the loop's hydro coordinates of (r0, r1, r2)
 *     cell = -1 when (a0, a1, a2) fails the loop's strict domain test, else the lowest-index cell whose closed extent holds the point
 *            cell < 0: n_unlocated += 1, the photon is in no bin
 *     beta = that cell's velocity at the azimuth of (r0, r1), as a re-location takes it
 *     e_lab = p0 * C_LIGHT   [erg]
 *     e_comv = lorentzBoost(beta, p)[0] * C_LIGHT   (mclib.c:302-407 in the loop's form, with the cell's staged Lorentz factor): the photon's energy
 *              in the local fluid frame
 *     terms:  w,  w*e_lab,  w*e_comv,  w*num_scatt,  w*temp[cell]
 * mode MCRAT_HIP_RADFIELD_CELLS:   bin = cell; n_bins = the frame's num_elements.
 * mode MCRAT_HIP_RADFIELD_SHELLS:  bin = ir * n_mu + imu, where bin k of an axis holds  edges[k] <= x < edges[k + 1]  for x = r and x = mu, decided
 *                                  by comparisons only; n_bins = n_r * n_mu.  A located photon outside either range adds to n_outside and to no bin.
 * Per bin six planes of 8 bytes: count (integer), W = sum w, WE_lab, WE_comv, WNS (w * num_scatt), WT (w * the cell's temperature); beside them
 * n_observable (counted photons), n_unlocated, n_outside: sum(count) + n_unlocated + n_outside == n_observable.  The photon temperature of a bin is
 * WE_comv / (W k_B xbar) (xbar = 2.701 for a black body, 3 for a Wien spectrum), the matter temperature the photons see WT / W: the caller's
 * quotients.  Counts are exact: the same as the same expressions in host code.  The five sums are added with floating-point atomics and are NOT
 * bit-reproducible from run to run; each is within (m + 2) * 2^-53 * sum|term| of the exact sum of its bin's m terms.
 *   mcrat_hip_radiation_field_bins  n_bins for these arguments -- what the caller's arrays must hold -- after the checks below (it needs the frame,
 *                                   not photons).
 *   mcrat_hip_radiation_field       one list: a stand-alone context, or a view of a pool (that list alone).  A pending advance is flushed first.
 *   mcrat_hip_pool_radiation_field  every list of a pool in one launch; it reads what mcrat_hip_pool_observe reads, a frame selected with
 *                                   mcrat_hip_pool_select_frame included.
 *   mcrat_hip_radiation_field_path  how the context's last call accumulated: 1 a copy of the planes per workgroup in LDS, flushed once (SHELLS whose
 *                                   edges and planes fit); 2 atomics straight into HBM (CELLS always; larger SHELLS); 0 none yet.
 *                                   MCRAT_HIP_RADFIELD_PATH=lds|global in the environment forces one (lds is refused where it cannot be had).
 * hydro: the context whose staged frame the photons are located in; NULL: ctx's own.  In a run that is the photons' slab: a caller who wants the whole
 * outflow stages the whole frame on a second context and passes it.  It must be on the same device with the same DIMENSIONS and GEOMETRY
 * (TAU_CALCULATION does not matter here).  No photon column changes; nearest_block_index is not touched.
 * MCRAT_HIP_EINVAL, with its own text in mcrat_hip_last_error, checked in this order: an unknown mode; SHELLS without r_edges or mu_edges; n_r or n_mu
 * < 1; n_r * n_mu overflowing an int; r_edges, then mu_edges, not finite; r_edges, then mu_edges, not strictly ascending; more edges than the kernel
 * can stage (about 10 000 values); MCRAT_HIP_RADFIELD_PATH neither lds nor global, lds with CELLS, lds with planes beyond LDS; a hydro context that does
 * not match.  Then MCRAT_HIP_ESTATE: no staged frame; no photons; the pool call on a context that is no pool and the one-list call on a pool.
 * Both calls synchronise before they return. */
#define MCRAT_HIP_RADFIELD_CELLS 0
#define MCRAT_HIP_RADFIELD_SHELLS 1
typedef struct mcrat_hip_radfield_bins {      /* inputs, host pointers; CELLS reads mode alone */
    int mode;
    int n_r;  const double *r_edges;          /* [n_r + 1] cm */
    int n_mu; const double *mu_edges;         /* [n_mu + 1] cosines of the polar angle, ascending */
} mcrat_hip_radfield_bins;
typedef struct mcrat_hip_radfield {           /* outputs: host pointers, each [n_bins] (SHELLS: r-major then mu), any may be NULL; and three counters */
    long long *count; double *w, *we_lab, *we_comv, *w_nscatt, *w_temp;
    long long n_observable, n_unlocated, n_outside;
} mcrat_hip_radfield;
int mcrat_hip_radiation_field_bins(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro /* or NULL */, const mcrat_hip_radfield_bins *bins, int *n_bins);
int mcrat_hip_radiation_field(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, mcrat_hip_radfield *out);
int mcrat_hip_pool_radiation_field(mcrat_hip_ctx *pool, const mcrat_hip_ctx *hydro, const mcrat_hip_radfield_bins *bins, mcrat_hip_radfield *out);
int mcrat_hip_radiation_field_path(const mcrat_hip_ctx *ctx);

/* the comoving radiation field: spectra, beaming and Eddington moments in the fluid frame ---
 * What mcrat_hip_radiation_field locates and boosts, kept: the resident photons located in ONE staged hydro frame, boosted into their cell's frame and
 * binned by position, fluid-frame energy and fluid-frame direction cosine about the flow.  A slot counts as for mcrat_hip_radiation_field.  For a
 * counted photon, in exactly this order, in IEEE double with correctly rounded division and square root and without contraction:
 *     r, mu                 as mcrat_hip_radiation_field has them
 *     cell                  as mcrat_hip_radiation_field locates it; cell < 0: n_unlocated += 1, the photon is in no bin
 *     beta[3], g            the cell's velocity at the azimuth of (r0, r1) and its staged Lorentz factor, as mcrat_hip_radiation_field obtains them
 *     bp    = (beta0*p1 + beta1*p2) + beta2*p3
 *     e_lab = p0 * C_LIGHT   [erg]
 *     e     = (g * (p0 - bp)) * C_LIGHT        the energy in the fluid frame [erg]: mcrat_hip_radiation_field's e_comv
 *     m     = ((p1*r0 + p2*r1) + p3*r2) / (p0 * r)     the lab cosine between the photon's direction and the radial direction
 *     b2    = (beta0*beta0 + beta1*beta1) + beta2*beta2
 *     a     = b2 > 0 ? ((bp / b) - b * p0) / (p0 - bp), with b = sqrt(b2)
 *                    : m
 *             the cosine, in the fluid frame, between the photon's direction and the flow direction: (p' . beta_hat) / p'0 in closed form, no
 *             Lorentz factor needed.  A cell at rest has no flow direction and its frame is the lab: the radial cosine.
 *     a, m  clamped into [-1, 1]; a NaN stays a NaN
 * Position bin s: mode MCRAT_HIP_COMOVING_CELLS: s = cell, n_s = the frame's num_elements; mode MCRAT_HIP_COMOVING_SHELLS: s = ir * n_mu + imu as
 * MCRAT_HIP_RADFIELD_SHELLS has it, n_s = n_r * n_mu.  ie and ia: bin k of an axis holds  edges[k] <= x < edges[k + 1]  for x = e and x = a, decided by
 * comparisons only.  bin = (s * n_e + ie) * n_a + ia.  A located photon outside any axis, or with a coordinate that is not a number, adds to
 * n_outside and to no bin.  The last a edge must lie above 1 for the forward pole (a == 1) to be counted.
 * Per bin eight planes of 8 bytes, each [n_s][n_e][n_a]: count (integer), w, we = w*e, wea = (w*e)*a, weaa = ((w*e)*a)*a, we_lab = w*e_lab,
 * wem = (w*e_lab)*m, wemm = ((w*e_lab)*m)*m; beside them n_observable, n_unlocated, n_outside:
 * sum(count) + n_unlocated + n_outside == n_observable.  The caller's quotients: J = sum we, H = sum wea, K = sum weaa over the a axis; K / J is the
 * Eddington factor (1/3 where the field is isotropic in the fluid frame, 1 where it streams) and H / J the mean cosine; the lab analogues about the
 * radial direction come from the last three planes summed over e and a.
 * Counts that do not hang on e or a -- n_observable, n_unlocated, the count summed over the e and a axes when their edges cover everything -- are
 * exact: the same as the same expressions in host code.  e and a are computed from the device's staged operands (the azimuth's reciprocal is the
 * loop's Newton form, gam is staged), so a photon within rounding of an e or a edge may fall on either side.  The seven sums are added with
 * floating-point atomics and are NOT bit-reproducible from run to run; each is within (m + 2) * 2^-53 * sum|term| of the exact sum of its bin's m
 * terms as the device computed them.
 *   mcrat_hip_comoving_field_bins   n_bins = n_s * n_e * n_a for these arguments -- what the caller's arrays must hold -- after the checks below (it
 *                                   needs the frame, not photons).
 *   mcrat_hip_comoving_field        one list: a stand-alone context, or a view of a pool (that list alone).  A pending advance is flushed first.
 *   mcrat_hip_pool_comoving_field   every list of a pool in one launch; it reads what mcrat_hip_pool_radiation_field reads, a frame selected with
 *                                   mcrat_hip_pool_select_frame included.
 *   mcrat_hip_comoving_field_path   how the context's last call accumulated: 1 a copy of the planes per workgroup in LDS, flushed once (SHELLS whose
 *                                   edges and planes fit); 2 atomics straight into HBM (CELLS always; larger SHELLS); 0 none yet.
 *                                   MCRAT_HIP_COMOVING_PATH=lds|global in the environment forces one (lds is refused where it cannot be had).
 * hydro: as for mcrat_hip_radiation_field -- NULL: ctx's own frame; a frame on another context must be on the same device with the same DIMENSIONS
 * and GEOMETRY.  No photon column changes.
 * MCRAT_HIP_EINVAL, with its own text in mcrat_hip_last_error, checked in this order: an unknown mode; e_edges or a_edges NULL, SHELLS without r_edges
 * or mu_edges; a count < 1; n_s * n_e * n_a overflowing an int (CELLS: once the frame is known, behind the checks below); r_edges, mu_edges,
 * e_edges, a_edges not finite, in that order; then the four not strictly ascending, in that order; more edges than the kernel can stage (about
 * 10 000 values); MCRAT_HIP_COMOVING_PATH neither lds nor global, lds with CELLS, lds with planes beyond LDS; a hydro context that does not match.
 * Then MCRAT_HIP_ESTATE: no staged frame; no photons; the pool call on a context that is no pool and the one-list call on a pool.
 * Both calls synchronise before they return. */
#define MCRAT_HIP_COMOVING_CELLS 0
#define MCRAT_HIP_COMOVING_SHELLS 1
typedef struct mcrat_hip_comoving_bins {      /* inputs, host pointers; CELLS reads neither n_r, r_edges nor n_mu, mu_edges */
    int mode;
    int n_r;  const double *r_edges;          /* [n_r + 1] cm */
    int n_mu; const double *mu_edges;         /* [n_mu + 1] cosines of the polar angle, ascending */
    int n_e;  const double *e_edges;          /* [n_e + 1] erg, in the fluid frame */
    int n_a;  const double *a_edges;          /* [n_a + 1] cosines about the flow in the fluid frame, ascending */
} mcrat_hip_comoving_bins;
typedef struct mcrat_hip_comoving {           /* outputs: host pointers, each [n_bins] (position-major, then e, then a), any may be NULL; and three counters */
    long long *count; double *w, *we, *wea, *weaa, *we_lab, *wem, *wemm;
    long long n_observable, n_unlocated, n_outside;
} mcrat_hip_comoving;
int mcrat_hip_comoving_field_bins(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro /* or NULL */, const mcrat_hip_comoving_bins *bins, int *n_bins);
int mcrat_hip_comoving_field(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, mcrat_hip_comoving *out);
int mcrat_hip_pool_comoving_field(mcrat_hip_ctx *pool, const mcrat_hip_ctx *hydro, const mcrat_hip_comoving_bins *bins, mcrat_hip_comoving *out);
int mcrat_hip_comoving_field_path(const mcrat_hip_ctx *ctx);

/* sky observers: mock observations from any direction, with images --------------
 * mcrat_hip_observe assumes an axisymmetric outflow: its observers are polar rings.  Here an observer is a direction anywhere on the sky with an
 * acceptance cone about it, the detection time comes from r.n, and the photon's position on the observer's sky plane may be two more axes of the
 * cube: resolved images.  Photons are 3-D Cartesian whatever the run's DIMENSIONS and GEOMETRY.
 * A slot counts as for mcrat_hip_observe: part of a list, weight != 0, type neither 'p' nor 'N'.  Observer o has a unit vector n = (n0, n1, n2)[o]
 * towards the observer, an acceptance cosine cos_acc[o] and, with image axes, two unit vectors ex = (x0, x1, x2)[o], ey = (y0, y1, y2)[o] that span
 * the sky plane.  In exactly this order, in IEEE double with correctly rounded division and without contraction:
 *     accepted:  ((p1*n0 + p2*n1) + p3*n2) >= p0*cos_acc        (cones may overlap; a photon counts for every observer that accepts it)
 *     e = p0 * C_LIGHT   [erg]
 *     t_det = time_now - (((r0*n0 + r1*n1) + r2*n2) / C_LIGHT)   [s]
 *     X = (r0*x0 + r1*x1) + r2*x2;   Y = (r0*y0 + r1*y1) + r2*y2   [cm]
 * Bin k of an axis holds  edges[k] <= x < edges[k + 1], decided by comparisons only.  The axes are time (n_t), energy (n_e) and, optionally, X
 * (n_x) and Y (n_y).  n_x == 0 && n_y == 0: no image axes -- X and Y are not computed and x0 .. y2, x_edges, y_edges may be NULL.  An accepted
 * photon outside any axis, or with a coordinate that is not a number, is in no bin and adds to n_outside[o].
 * The cube: seven planes per bin as mcrat_hip_observe has them -- count (integer), W = sum w, WE = sum w*e, I, Q, U, V = sum w*s0 .. s3 (zero with
 * stokes_switch off) -- each [n_obs][n_t][n_e][n_y][n_x] with x fastest ([n_obs][n_t][n_e] without image axes); beside it n_accepted[n_obs] and
 * n_outside[n_obs].  Every output pointer may be NULL.
 * The Stokes frame: Q and U are summed as the photons store them, as mcrat_hip_observe does.  MCRaT defines a photon's Stokes frame from its own
 * direction and the polar axis (mcrat_scattering.c, findXY); for photons inside a narrow cone about n those frames coincide to first order in the
 * cone's half-angle, at any azimuth phi.  The natural sky axes of an observer at (theta, phi) are ey = phi_hat = (-sin phi, cos phi, 0) and
 * ex = theta_hat = (cos theta cos phi, cos theta sin phi, -sin theta), so that ex x ey = n.
 * Counts are exact: the same as the same expressions in host code.  The sums are added with floating-point atomics and are NOT bit-reproducible
 * from run to run; each is within (m + 2) * 2^-53 * sum|term| of the exact sum of its bin's m terms.
 * MCRAT_HIP_EINVAL, each with its own text in mcrat_hip_last_error, checked in this order: n_obs, n_t or n_e < 1; n_x and n_y neither both 0 nor
 * both >= 1; the product of the five counts overflowing an int; a direction that is not finite; a direction that is not unit,
 * |((n0*n0 + n1*n1) + n2*n2) - 1| > 1e-12; cos_acc not finite or outside [-1, 1]; with image axes: the sky-plane vectors NULL, not finite, not
 * unit, or any of |ex.n|, |ey.n|, |ex.ey| above 1e-12; t_edges not finite, then not strictly ascending, the same for e_edges, x_edges, y_edges; more
 * edges and observers than the kernel can stage (about 9 000 values together); MCRAT_HIP_SKY_PATH neither lds nor global; lds forced for a cube
 * that does not fit.  (1e-12 is a condition on the inputs: vectors built from cos and sin in double miss it by three orders of magnitude.)
 *   mcrat_hip_observe_sky        one list: a stand-alone context, or a view of a pool (that list alone); time_now is the list's clock.  A pending
 *                                advance is flushed first.  MCRAT_HIP_ESTATE without photons, and on a pool.
 *   mcrat_hip_pool_observe_sky   every list of a pool in one launch, each with its own clock time_now[r]; it reads exactly what
 *                                mcrat_hip_pool_observe reads, and like it flushes nothing a view holds pending.  MCRAT_HIP_ESTATE on a context
 *                                that is no pool.
 *   mcrat_hip_observe_sky_path   how the context's last sky observation was accumulated: 1 a copy of the cube per workgroup in LDS, flushed once
 *                                (light curves, small images); 2 atomics straight into the cube in HBM (images); 0 none yet.
 *                                MCRAT_HIP_SKY_PATH=lds|global in the environment forces one.
 * Both calls synchronise before they return.  No photon column changes. */
typedef struct mcrat_hip_sky_observer {  /* inputs, host pointers */
    int n_obs; const double *n0, *n1, *n2, *cos_acc;               /* [n_obs] */
    const double *x0, *x1, *x2, *y0, *y1, *y2;                     /* [n_obs]: ex and ey; read with image axes only */
    int n_t;   const double *t_edges;                              /* [n_t + 1] seconds */
    int n_e;   const double *e_edges;                              /* [n_e + 1] erg */
    int n_x;   const double *x_edges;                              /* [n_x + 1] cm; n_x == n_y == 0: no image axes */
    int n_y;   const double *y_edges;                              /* [n_y + 1] cm */
} mcrat_hip_sky_observer;
typedef struct mcrat_hip_sky_observation {   /* outputs, host pointers, each [n_obs * n_t * n_e * max(n_y, 1) * max(n_x, 1)]; any may be NULL */
    long long *count; double *w, *we, *i, *q, *u, *v;
    long long *n_accepted, *n_outside;   /* [n_obs] */
} mcrat_hip_sky_observation;
int mcrat_hip_observe_sky(mcrat_hip_ctx *ctx, const mcrat_hip_sky_observer *obs, double time_now, mcrat_hip_sky_observation *out);
int mcrat_hip_pool_observe_sky(mcrat_hip_ctx *pool, const mcrat_hip_sky_observer *obs, const double *time_now /* [n_ranks] */, mcrat_hip_sky_observation *out);
int mcrat_hip_observe_sky_path(const mcrat_hip_ctx *ctx);

/* escape-weighted sky observations: optical depth as an axis of the cube ---------
 * mcrat_hip_observe_sky counts a photon at tau = 30 to the edge of the outflow exactly like one that is already free.  Here every photon that an
 * observer accepts is first marched to the edge of a staged frame, and its optical depth becomes one more axis of the cube; beside the raw sums the
 * cube holds the sums weighted with exp(-tau).
 * What exp(-tau) means: for a photon at x moving along p_hat through ONE frozen frame it is the probability that its current flight leaves the frame
 * without another scattering; tau is the straight-line optical depth to the edge, exactly as mcrat_hip_sightline_* define it.  The accepted
 * photons move within the cone about n, so sum w * exp(-tau) per (observer, time, energy[, pixel]) is the expected signal already streaming towards
 * that observer, and the tau axis shows from which depth that signal comes.  This is NOT a peel-off estimator towards n: the direction is the
 * photon's own.
 * Counted slots: as for mcrat_hip_observe.  Acceptance and axes: observer o accepts a photon by the rule of mcrat_hip_observe_sky, and its e, t_det
 * and (X, Y) are that call's, the same expressions in the same order; `sky` is read exactly as mcrat_hip_observe_sky reads its struct.
 * The march: a slot accepted by at least one observer is marched once, from (r0, r1, r2) along (p0 .. p3) through the staged frame of `hydro` (NULL:
 * the context's own), by the sightline definition above with march.step_frac, h_min, max_steps and tau_stop (march.surface_level is not read); it
 * ends in tau and a status.  A slot nobody accepts is not marched.
 * For every observer o that accepts the photon: status OPAQUE adds to n_opaque[o]; STEP_CAP or OFF_TABLE adds to n_unresolved[o]; LEFT_MESH -- tau
 * is the optical depth to the edge -- goes to bin (o, itau, it, ie[, iy, ix]), every axis decided by  edges[k] <= x < edges[k + 1]  through
 * comparisons only; a LEFT_MESH photon outside any axis, or with a coordinate (tau included) that is not a number, adds to n_outside[o].  A photon
 * that starts outside the frame has tau = 0 exactly and is a legitimate member of a bin that holds 0.
 * The cube: nine planes of 8 bytes per bin -- count (integer), W = sum w, WE = sum w*e, I, Q, U, V = sum w*s0 .. s3 (zero with stokes_switch off) as
 * mcrat_hip_observe_sky has them, WX = sum w*x and WEX = sum (w*e)*x with x = exp(-tau) -- each [n_obs][n_tau][n_t][n_e][n_y][n_x] with x fastest
 * ([n_obs][n_tau][n_t][n_e] without image axes).  Per observer:  sum of count over o's bins + n_outside[o] + n_opaque[o] + n_unresolved[o] ==
 * n_accepted[o].  Per call:  n_status[1] + .. + n_status[4] == n_selected <= n_observable; n_selected is the number of counted slots that at least
 * one observer accepts, which is the number of rays marched, n_status[s] the marched rays that ended with sightline status s (n_status[0] is 0).
 * Exactness: counts that do not hang on tau are exact, as in mcrat_hip_observe_sky.  tau is the sightline kernel's tau bit for bit -- both kernels
 * call one march step --, so the cube's counts equal those of mcrat_hip_sightline_photons' tau binned by the same rules.  The sums are added with
 * floating-point atomics and are NOT bit-reproducible; each is within (m + 2) * 2^-53 * sum|term| of the exact sum of its terms as the device
 * computed them.
 * MCRAT_HIP_EINVAL, each with its own text in mcrat_hip_last_error, prefixed "observe_escaping:", checked in this order: the checks of
 * mcrat_hip_observe_sky on `sky`, in that call's order up to the edges; n_tau < 1; the product of the six counts overflowing an int; tau_edges not
 * finite, then not strictly ascending; the sightline checks of step_frac, h_min, max_steps, tau_stop in the sightline order; more edges and
 * observers than the kernel can stage; MCRAT_HIP_ESCAPE_PATH neither lds nor global; lds forced for a cube that does not fit; a `hydro` context on
 * another device or with other DIMENSIONS, GEOMETRY or TAU_CALCULATION.  Then MCRAT_HIP_ESTATE: no staged frame; TABLE without a table.
 *   mcrat_hip_observe_escaping        one list: a stand-alone context, or a view of a pool (that list alone); time_now is the list's clock.  A
 *                                     pending advance is flushed first.  MCRAT_HIP_ESTATE without photons, and on a pool, before any other check.
 *   mcrat_hip_pool_observe_escaping   every list of a pool, each with its own clock time_now[r]; it reads exactly what mcrat_hip_pool_observe_sky
 *                                     reads, and like it flushes nothing a view holds pending.  MCRAT_HIP_ESTATE on a context that is no pool.
 *   mcrat_hip_observe_escaping_path   how the context's last escape-weighted observation was accumulated: 1 a copy of the cube per workgroup in
 *                                     LDS, flushed once; 2 atomics straight into the cube in HBM; 0 none yet.  MCRAT_HIP_ESCAPE_PATH=lds|global in
 *                                     the environment forces one.
 * Both calls synchronise once, before they return.  No photon column changes. */
typedef struct mcrat_hip_escape_observer {      /* inputs, host pointers */
    mcrat_hip_sky_observer sky;                 /* observers, cones, t/e edges, optional image axes: read exactly as mcrat_hip_observe_sky reads them */
    int n_tau; const double *tau_edges;         /* [n_tau + 1], finite, strictly ascending */
    mcrat_hip_sightline_params march;           /* step_frac, h_min, max_steps, tau_stop as the sightline calls read them; surface_level is not read */
} mcrat_hip_escape_observer;
typedef struct mcrat_hip_escape_observation {   /* outputs, host pointers; any may be NULL */
    long long *count; double *w, *we, *i, *q, *u, *v, *wx, *wex;   /* each [n_obs][n_tau][n_t][n_e][n_y][n_x], x fastest; without image axes [n_obs][n_tau][n_t][n_e] */
    long long *n_accepted, *n_outside, *n_opaque, *n_unresolved;   /* [n_obs] */
    long long n_observable, n_selected, n_status[5];               /* counted slots; slots at least one observer accepts (= rays marched); the marched rays per sightline status */
} mcrat_hip_escape_observation;
int mcrat_hip_observe_escaping(mcrat_hip_ctx *ctx, const mcrat_hip_ctx *hydro /* or NULL */, const mcrat_hip_escape_observer *obs, double time_now, mcrat_hip_escape_observation *out);
int mcrat_hip_pool_observe_escaping(mcrat_hip_ctx *pool, const mcrat_hip_ctx *hydro, const mcrat_hip_escape_observer *obs, const double *time_now /* [n_ranks] */, mcrat_hip_escape_observation *out);
int mcrat_hip_observe_escaping_path(const mcrat_hip_ctx *ctx);

/* sky polarimetry: observer-frame Stokes sums and a resampling axis ---------------
 * A sky observation (mcrat_hip_observe_sky) whose Q and U can be summed in the observer's sky-plane frame and whose cube has a replica axis behind
 * the observer: jackknife groups for standard errors, Poisson-bootstrap replicas for the distribution of any derived quantity (polarisation degree
 * and angle, <E> = WE / W, light-curve points).  Which slots are counted, acceptance, e, t_det, (X, Y), the bin rule, n_accepted and n_outside are
 * mcrat_hip_observe_sky's, unchanged; `sky` is read exactly as that call reads its struct.
 * The cube: the seven planes count, W, WE, I, Q, U, V, each [n_obs][n_rep][n_t][n_e][n_y][n_x] with x fastest ([n_obs][n_rep][n_t][n_e] without
 * image axes).  An accepted, binned photon adds to replica rho:  k  to count and  (double)k * term  to each sum, term exactly mcrat_hip_observe_sky's
 * -- w, w*e, w*s0 .. s3, with (s1, s2) possibly rotated (below).  k = k(photon identity, rho) does not depend on the observer.
 * Photon identity: (rank, slot) -- rank the list's index in its pool (the view's rank for a view, slot / rank_stride in a pool call, 0 for a
 * stand-alone context), slot the index within the list; a view and its pool give a photon the same k.  All draws are words w[0 .. 3] of the
 * Philox4x32-10 block with counter {slot, rank, block, 2 | mode << 8} and key `seed` (2: this product's purpose word):
 *   MCRAT_HIP_RESAMPLE_NONE        n_rep == 1, k = 1.
 *   MCRAT_HIP_RESAMPLE_JACKKNIFE   n_rep = G >= 2 disjoint groups: block 0, g = ((uint64_t)w[0] * G) >> 32, k = [rho == g]; entry g holds group g's
 *                                  own sums, so the sum over the entries is the sky observation.
 *   MCRAT_HIP_RESAMPLE_BOOTSTRAP   n_rep = B + 1 >= 2: entry 0 is the sample itself (k = 1); for rho >= 1, j = rho - 1, the block is j >> 2, the word
 *                                  w[j & 3] and k = #{m : word >= T_m}, T_m = floor(2^32 * sum_{i <= m} exp(-1) / i!) for m = 0 .. 11 (T_0 =
 *                                  1580030168): a Poisson(1) draw, k <= 12, with a truncation bias below 2^-31.
 * Integer arithmetic throughout: every count is exactly reproducible on the host.
 * The Stokes frame.  MCRAT_HIP_STOKES_AS_STORED: Q and U are summed as the photons store them, as mcrat_hip_observe_sky does -- each in the
 * photon's own frame (theta_hat, phi_hat of its direction), which turns against the observer's by about alpha * cot(theta_obs) for a photon alpha
 * off the line of sight.  MCRAT_HIP_STOKES_SKY_PLANE: for every accepted (photon, observer) pair (Q, U) are carried from the photon's frame to the
 * observer's with MCRaT's own rule (findPhi and mullerMatrixRotation, mcrat_scattering.c), written so that it stays well conditioned near zero
 * angle.  With p = (p1, p2, p3) and ey the observer's second sky-plane vector, in exactly this order, IEEE double, correctly rounded, no contraction:
 *     rho2 = p1*p1 + p2*p2;   pn = sqrt(rho2 + p3*p3);   d = p2*ey0 - p1*ey1;   s = (rho2*ey2 - p3*(p1*ey0 + p2*ey1)) / pn;
 *     h = sqrt(d*d + s*s);   c = d / h;   sg = s / h;   c2 = c*c - sg*sg;   s2 = (-2.0*sg) * c;
 *     Q' = Q*c2 - U*s2;   U' = Q*s2 + U*c2;   I and V are unchanged
 * (d and s are y_ph . y_new and x_ph . y_new up to one positive factor: y_ph ~ (p2, -p1, 0), x_ph = y_ph x p_hat, y_new ~ ey - (ey . p_hat) p_hat).
 * When h is 0 or not finite (p parallel to the polar axis, or to ey) the pair's Q and U are added as stored and n_frame_undefined[o] counts the
 * accepted pair, binned or not.  SKY_PLANE needs ex and ey even without image axes.  With stokes_switch off there is nothing to rotate: I, Q, U, V
 * stay zero and n_frame_undefined stays 0.
 * The sense of U: a photon at azimuth phi_p infinitesimally off the axis, with stored (Q, U) = (1, 0), seen by the on-axis observer with
 * ex = x_hat, ey = y_hat, contributes (cos 2 phi_p, -sin 2 phi_p).  It is MCRaT's sense of U.
 * Exactness: counts and counters are exact; each sum is within (m + 2) * 2^-53 * sum|k * term| of the exact sum of its bin's m terms k * term.
 * MCRAT_HIP_EINVAL, each with its own text in mcrat_hip_last_error, prefixed "observe_sky_resampled:", checked in this order: the checks of
 * mcrat_hip_observe_sky on `sky`, in that call's order up to the edges; mode; stokes_frame; n_rep (NONE: not 1; otherwise < 2); the product of the
 * six counts overflowing an int; SKY_PLANE without ex and ey, or with ex, ey not finite, not unit or not orthogonal to 1e-12; more edges and
 * observers than the kernel can stage; MCRAT_HIP_RESAMPLE_PATH none of lds, sliced, global; a forced path that does not fit.
 *   mcrat_hip_observe_sky_resampled        one list: a stand-alone context, or a view of a pool (that list alone); time_now is the list's clock.  A
 *                                          pending advance is flushed first.  MCRAT_HIP_ESTATE without photons, and on a pool.
 *   mcrat_hip_pool_observe_sky_resampled   every list of a pool in one launch, each with its own clock time_now[r]; it reads exactly what
 *                                          mcrat_hip_pool_observe_sky reads, and like it flushes nothing a view holds pending.  MCRAT_HIP_ESTATE on
 *                                          a context that is no pool.
 *   mcrat_hip_observe_sky_resampled_path   how the context's last such observation was accumulated: 1 a copy of the whole cube per workgroup in LDS;
 *                                          3 sliced -- the replica axis cut into slices, a workgroup owns one slice's part of the cube in LDS, walks
 *                                          all slots and adds the replicas of its slice; 2 atomics straight into the cube in HBM; 0 none yet.
 *                                          MCRAT_HIP_RESAMPLE_PATH=lds|sliced|global in the environment forces one.
 * Both calls synchronise once, before they return.  No photon column changes. */
#define MCRAT_HIP_RESAMPLE_NONE      0   /* n_rep == 1: a sky observation, with the Stokes frame below */
#define MCRAT_HIP_RESAMPLE_JACKKNIFE 1   /* n_rep = G >= 2 disjoint groups; entry g holds group g's own sums */
#define MCRAT_HIP_RESAMPLE_BOOTSTRAP 2   /* n_rep = B + 1 >= 2; entry 0 is the sample itself, entries 1..B are Poisson(1) resamples */
#define MCRAT_HIP_STOKES_AS_STORED   0
#define MCRAT_HIP_STOKES_SKY_PLANE   1
typedef struct mcrat_hip_resample_observer {      /* inputs, host pointers */
    mcrat_hip_sky_observer sky;                   /* read exactly as mcrat_hip_observe_sky reads it */
    int mode, n_rep, stokes_frame;
    uint64_t seed;
} mcrat_hip_resample_observer;
typedef struct mcrat_hip_resample_observation {   /* outputs, host pointers; any may be NULL */
    long long *count; double *w, *we, *i, *q, *u, *v;        /* each [n_obs][n_rep][n_t][n_e][n_y][n_x], x fastest */
    long long *n_accepted, *n_outside, *n_frame_undefined;   /* [n_obs] */
} mcrat_hip_resample_observation;
int mcrat_hip_observe_sky_resampled(mcrat_hip_ctx *ctx, const mcrat_hip_resample_observer *obs, double time_now, mcrat_hip_resample_observation *out);
int mcrat_hip_pool_observe_sky_resampled(mcrat_hip_ctx *pool, const mcrat_hip_resample_observer *obs, const double *time_now /* [n_ranks] */, mcrat_hip_resample_observation *out);
int mcrat_hip_observe_sky_resampled_path(const mcrat_hip_ctx *ctx);

/* detected-photon event lists: time-ordered rows per observer ---------------------
 * The list of photons each observer detects, one row per accepted (photon, observer) pair inside a window of detection time and energy, made where
 * the photons live: what ProcessMCRaT calls an ObservedPhotonList.  It is what comes before any binning -- T90 from the cumulative fluence, bins of
 * equal counts, Bayesian blocks, unbinned fits, other edges without another pass over the photons, a look at single photons.
 * Counted slots: as for mcrat_hip_observe.
 * Observers: n_obs, n0 n1 n2 (unit, towards the observer) and cos_acc as in mcrat_hip_sky_observer.  The sky-plane vectors x0 .. x2 (ex) and
 * y0 .. y2 (ey) are optional: they are read when all six are given, and only then are the X and Y columns produced; MCRAT_HIP_STOKES_SKY_PLANE
 * needs them.  Without them the X and Y output pointers must be NULL.
 * Acceptance, e, t_det, (X, Y): observer o accepts a photon by the rule of mcrat_hip_observe_sky, and e = p0 * C_LIGHT, t_det and (X, Y) are that
 * call's -- the same expressions in the same order, evaluated by the same functions.
 * The window:  t_lo <= t_det < t_hi  and  e_lo <= e < e_hi, by comparisons only; a bound may be -inf or +inf.  An accepted pair outside the window,
 * or with a coordinate that is not a number, adds to n_outside[o]; every other accepted pair is an event:
 * n_events[o] + n_outside[o] == n_accepted[o].
 * The Stokes frame: stokes_frame is MCRAT_HIP_STOKES_AS_STORED -- s1 and s2 as the photon stores them -- or MCRAT_HIP_STOKES_SKY_PLANE -- (s1, s2)
 * carried into the observer's frame by the rotation of mcrat_hip_observe_sky_resampled, per pair.  n_frame_undefined[o] counts the accepted pairs,
 * inside the window or not, for which that rotation is undefined; their rows hold s1 and s2 as stored.  With stokes_switch off the s0 .. s3 columns
 * are zero and n_frame_undefined stays 0.
 * Rows: the columns are optional output pointers, each [capacity]: rank and slot (int) -- the photon's identity exactly as
 * mcrat_hip_observe_sky_resampled defines it, so a view and its pool agree --; t, e, w (the weight), s0, s1, s2, s3, X, Y, num_scatt (double); type
 * (char).  offsets [n_obs + 1]: observer o's rows are [offsets[o], offsets[o + 1]); offsets[n_obs] == n_total.
 * Order.  MCRAT_HIP_EVENTS_BY_PHOTON: rows ordered by (observer, rank, slot).  MCRAT_HIP_EVENTS_BY_TIME: by (observer, key(t), rank, slot), key(t)
 * the usual order-preserving map of the double's bits to a uint64_t: with the sign bit set all bits are inverted, otherwise the sign bit is set.
 * So -0.0 sorts before +0.0, -inf is a legal key, and a NaN never reaches a row.  The order is fully specified and every value of a row is one of
 * the documented IEEE expressions: every output is bit-reproducible from run to run.
 * Capacity: handled on the device, with no host round trip between the kernels.  Rows at index >= capacity are not written; n_events, n_accepted,
 * n_outside, n_frame_undefined, offsets and n_total are always exact.  When n_total > capacity the call returns MCRAT_HIP_EREFUSED with its own text;
 * the row outputs are then unspecified -- no partial list is to be trusted.  capacity == 0 with all row pointers NULL is the counting call: it
 * returns 0 whatever n_total.  Each row column is copied back in full, `capacity` entries; those behind n_total are unspecified.
 * The sort (BY_TIME): a stable LSD radix sort over 8-bit digits of key(t), then of the observer index.  A digit that is the same in all keys -- the
 * OR and the AND of all keys agree in it -- is skipped on the device.  key_or and key_and return the two masks (0 and ~0 for an empty list),
 * sort_passes_run and sort_passes_skipped what followed from them (both 0 for BY_PHOTON, for an empty list and for one that did not fit).
 * MCRAT_HIP_EINVAL, each with its own text in mcrat_hip_last_error, prefixed "observe_events:", checked in this order: the checks of
 * mcrat_hip_observe_sky on the observers in that call's order up to the cosines -- n_obs < 1, a direction not finite, not unit, cos_acc no number in
 * [-1, 1] --; order; stokes_frame; ex and ey given but not finite, not unit or not orthogonal to 1e-12; SKY_PLANE without them; X or Y pointers
 * without them; a bound of the window that is not a number, then t_lo >= t_hi or e_lo >= e_hi; capacity < 0, then capacity beyond INT_MAX; more than
 * 512 observers.
 *   mcrat_hip_observe_events        one list: a stand-alone context, or a view of a pool (that list alone); time_now is the list's clock.  A
 *                                   pending advance is flushed first.  MCRAT_HIP_ESTATE without photons, and on a pool.
 *   mcrat_hip_pool_observe_events   every list of a pool, each with its own clock time_now[r]; it reads exactly what mcrat_hip_pool_observe_sky
 *                                   reads, and like it flushes nothing a view holds pending.  MCRAT_HIP_ESTATE on a context that is no pool.
 * Both calls synchronise once, before they return.  No photon column changes. */
#define MCRAT_HIP_EVENTS_BY_PHOTON 0
#define MCRAT_HIP_EVENTS_BY_TIME   1
typedef struct mcrat_hip_events_observer {        /* inputs, host pointers */
    int n_obs; const double *n0, *n1, *n2, *cos_acc;               /* [n_obs] */
    const double *x0, *x1, *x2, *y0, *y1, *y2;                     /* [n_obs]: ex and ey; all six, or NULL */
    double t_lo, t_hi, e_lo, e_hi;                                 /* the window: seconds, erg */
    int order, stokes_frame;
    long long capacity;                                            /* rows the column outputs have room for */
} mcrat_hip_events_observer;
typedef struct mcrat_hip_events {                 /* outputs, host pointers; any may be NULL */
    int *rank, *slot;                                              /* [capacity] */
    double *t, *e, *w, *s0, *s1, *s2, *s3, *X, *Y, *num_scatt;     /* [capacity] */
    char *type;                                                    /* [capacity] */
    long long *offsets;                                            /* [n_obs + 1] */
    long long *n_events, *n_accepted, *n_outside, *n_frame_undefined;   /* [n_obs] */
    long long n_total;
    unsigned long long key_or, key_and;
    int sort_passes_run, sort_passes_skipped;
} mcrat_hip_events;
int mcrat_hip_observe_events(mcrat_hip_ctx *ctx, const mcrat_hip_events_observer *obs, double time_now, mcrat_hip_events *out);
int mcrat_hip_pool_observe_events(mcrat_hip_ctx *pool, const mcrat_hip_events_observer *obs, const double *time_now /* [n_ranks] */, mcrat_hip_events *out);

/* spectral fits: Band function and cutoff power law, every row of a cube at once ---
 * What comes after a spectrum: every row of a [n_spec][n_e] pair (count, w) -- an observer, a time bin and a jackknife or bootstrap entry each, as
 * the observe calls give them -- fitted to a cutoff power law (MCRAT_HIP_FIT_COMP) or a Band function (MCRAT_HIP_FIT_BAND) by a deterministic,
 * derivative-free chi^2 search.  The arrays are host arrays: the call uploads them, fits on the device -- a wavefront per spectrum -- and copies the
 * columns back.  It reads no photon and no frame; any context will do.
 * Data.  Bin i has the edges e_edges[i], e_edges[i + 1] (erg) and the width dE_i.  log_e[i] = ln(E_i / e_piv) at the geometric centre is an input,
 * so that every implementation sees the same bits.  y_i = w_i / dE_i, the weight g_i = count_i / y_i^2 (sigma_i = y_i / sqrt(count_i)).  A bin is
 * used iff count_i >= min_count, w_i is finite and w_i > 0; the used bins are compacted in bin order.  With fewer used bins than parameters + 1
 * (COMP 2, BAND 3) the status is MCRAT_HIP_FIT_TOO_FEW_BINS, the double outputs are NaN and no search runs.
 * Models, in u = (alpha, lambda, beta), lambda = ln(E_pk / e_piv): with x_i = (2 + alpha) exp(L_i - lambda), COMP is ln m_i = alpha L_i - x_i; BAND
 * the same where x_i < alpha - beta and ln m_i = (alpha - beta)(ln(alpha - beta) - ln(2 + alpha) + lambda - 1) + beta L_i elsewhere.  A candidate
 * with 2 + alpha <= 0 or (BAND) alpha <= beta has chi^2 = +inf.  The amplitude is profiled out: A = sum g y m / sum g m^2, chi^2 = sum g (y - A m)^2,
 * two passes over the used bins in order.  exp and log are fixed sequences of IEEE operations (fit_plan.hpp: fit_exp, fit_log; within 4 ulp).
 * Search.  Round 0: the cell centres of a grid of g_alpha x g_lambda x g_beta cells over the bounds (COMP: g_beta counts as 1).  Rounds
 * 1 .. n_rounds: 4 x 4 x 4 (BAND) or 8 x 8 (COMP) cell centres of a box whose side is the previous side times shrink, centred on the best candidate
 * of all rounds so far and shifted, not clipped, into the bounds.  Best: the lowest chi^2; among equals the earliest round, then the lowest index
 * (alpha fastest).  Every operation and its order are fit_plan.hpp's: the outputs are bit-reproducible, on the device, in g++ and in NumPy.
 * Outputs, [n_spec] each, any may be NULL: alpha; beta (NaN for COMP); e_peak = e_piv * exp(lambda); amplitude; chi2; n_used; dof = n_used -
 * parameters; status, a bit set: TOO_FEW_BINS; AT_BOUND_ALPHA, _LAMBDA, _BETA -- the result lies within one cell of the last round of a bound --;
 * NO_FINITE_CANDIDATE -- no candidate had a finite chi^2: chi2 is +inf, the other doubles NaN.
 * MCRAT_HIP_EINVAL, each with its own text in mcrat_hip_last_error, prefixed "fit_spectra:", checked in this order: model; a NULL array; n_e < 1 or
 * above 512; an edge not finite, the edges not strictly ascending, not positive; log_e not finite; e_piv not positive and finite; a bound not
 * finite, lo >= hi, no candidate allowed (alpha_hi <= -2, or BAND alpha_hi <= beta_lo); a grid count < 1, the coarse grid above 2^20 candidates;
 * n_rounds outside [0, 4096]; shrink outside (0.25, 1); min_count < 1; n_spec outside [0, INT_MAX].  COMP does not read beta's bounds.
 * The call synchronises the stream twice: before it sizes its device block, and before it returns. */
#define MCRAT_HIP_FIT_COMP 0
#define MCRAT_HIP_FIT_BAND 1
#define MCRAT_HIP_FIT_TOO_FEW_BINS         1
#define MCRAT_HIP_FIT_AT_BOUND_ALPHA       2
#define MCRAT_HIP_FIT_AT_BOUND_LAMBDA      4
#define MCRAT_HIP_FIT_AT_BOUND_BETA        8
#define MCRAT_HIP_FIT_NO_FINITE_CANDIDATE 16
typedef struct mcrat_hip_fit_args {               /* inputs, host pointers */
    int model;
    long long n_spec; int n_e;
    const long long *count; const double *w;                       /* [n_spec][n_e] */
    const double *e_edges, *log_e;                                 /* [n_e + 1] (erg), [n_e] */
    double e_piv;                                                  /* erg */
    double alpha_lo, alpha_hi, lambda_lo, lambda_hi, beta_lo, beta_hi;
    int g_alpha, g_lambda, g_beta, n_rounds;
    double shrink;
    long long min_count;
} mcrat_hip_fit_args;
typedef struct mcrat_hip_fit_result {             /* outputs, host pointers; any may be NULL */
    double *alpha, *beta, *e_peak, *amplitude, *chi2;              /* [n_spec] */
    int *n_used, *dof, *status;                                    /* [n_spec] */
} mcrat_hip_fit_result;
int mcrat_hip_fit_spectra(mcrat_hip_ctx *ctx, const mcrat_hip_fit_args *args, mcrat_hip_fit_result *out);

/* introspection used by bench.py / tests -------------------------------------- */
int mcrat_hip_synchronize(mcrat_hip_ctx *ctx);
/* HBM held by the context: photons, staged frame, cell-lookup grid, loop state and the device blocks of all nine analysis products -- observe,
 * observe_sky, sightline_*, radiation_field, comoving_field, observe_escaping, observe_sky_resampled, observe_events and fit_spectra (the blocks of radiation_field
 * and of observe_sky were left out before they became one array).  A view holds no analysis block of its own: it uses its pool's, and they count there. */
size_t mcrat_hip_device_bytes(const mcrat_hip_ctx *ctx);
int mcrat_hip_lookup_cell(mcrat_hip_ctx *ctx, int n, const double *a0, const double *a1, const double *a2, int *cell_out); /* device cell search == findContainingBlock geometry.c:350 */
/* The staged frame's covered-octant table (one int per lookup bucket and octant, bucket-major: the cell that covers the octant, or -1): returns its
 * number of entries -- 0: the frame's grid has none (a log-mapped axis, above the size cap, MCRAT_HIP_NO_COVERED), negative: an MCRAT_HIP_E* code --
 * and copies the first min(entries, cap) to out (out may be NULL with cap 0). */
long long mcrat_hip_covered_octants(mcrat_hip_ctx *ctx, int *out, long long cap);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MCRAT_HIP_H */
