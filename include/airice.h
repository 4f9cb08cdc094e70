/*
 * airice.h -- C-ABI of libairice.so, the MI355X (gfx950) implementation of the
 * uzairlatif90/AirIceRayTracing hot path:
 *   - MultiRayAirIceRefraction table generation  (MakeRayTracingTable,
 *     MultiRayAirIceRefraction.cc:2019-2158, one ray = GetRayTracingSolutions .cc:1796-2017)
 *   - per-(Tx,Rx) launch-angle root finding      (Air2IceRayTracing .cc:1464-1616 and the
 *     CoREAS entry GetHorizontalDistanceToIntersectionPoint .cc:945-989)
 *   - the pythonwrapper ctypes surface           (Py_TraceIceToAir, pythonwrapper/TraceIceToAir.C:75-79)
 *
 * Plain C types only (no HIP / torch types).  Device pointers are hipMalloc'd (or
 * torch CUDA tensors' data_ptr) and `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  All *_launch entry points are stream-ordered and
 * asynchronous; *_host entry points copy, launch and synchronise.
 *
 * Errors: every int-returning function returns AIRICE_OK (0) or a negative
 * AIRICE_E* code; airice_last_error() gives a message.  Numerical failure modes
 * follow the reference (NaN propagation, -1000 / zeroed outputs), see DESIGN.md.
 *
 * Thread safety: the reference library is not reentrant (namespace statics,
 * MultiRayAirIceRefraction.h:33-81).  Here the medium is an explicit value
 * (airice_medium) and every batch entry point is reentrant.
 */
#ifndef AIRICE_H
#define AIRICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIRICE_OK 0
#define AIRICE_EINVAL (-1)
#define AIRICE_EIO (-2)
#define AIRICE_EHIP (-3)
#define AIRICE_ENOMEM (-4)

/* Variant of the reference namespace whose numerics are reproduced. */
#define AIRICE_VARIANT_MULTIRAY 0  /* MultiRayAirIceRefraction:: (pi = 3.1415927, .h:29) */
#define AIRICE_VARIANT_PYWRAPPER 1 /* AirIceRayTracing::        (pi = 4*atan(1), pythonwrapper .h:25) */

/* Per-query solve status bits (GSL 2.x bisection semantics). */
/* AIRICE_SOLVE_NONFINITE_END: f(lo) or f(hi) is non-finite, so gsl_root_fsolver_set returns before
 * storing f_lower/f_upper and the reference's next gsl_root_fsolver_iterate reads uninitialised
 * malloc memory.  The reference's result on such a row is undefined; this
 * library (and the oracle) model a zero-filled solver state, which is deterministic but NOT what
 * real GSL returns -- a consumer comparing against GSL must mask these rows (about 0.7 % of the
 * cfg3 distribution), as the parity tests do.  AIRICE_SOLVE_BAD_BRACKET and
 * AIRICE_SOLVE_NO_AIR_LAYER rows are undefined in the reference in the same sense. */
#define AIRICE_SOLVE_NONFINITE_END 1 /* f(lo) or f(hi) non-finite: reference reads uninitialised GSL state */
#define AIRICE_SOLVE_BAD_BRACKET 2   /* lo > hi: gsl_root_fsolver_set fails */
#define AIRICE_SOLVE_STALE_MID 4     /* a bisection midpoint gave non-finite f: root frozen */
#define AIRICE_SOLVE_PROBED 8        /* bracket-probe loop ran (.cc:1490-1511) */
#define AIRICE_SOLVE_MAXITER 16      /* 40 iterations, interval test never passed */
#define AIRICE_SOLVE_NO_AIR_LAYER 32 /* no air layer between Tx and the ice */

/* Medium: the GDAS layered atmosphere reduced to its run-time parameters plus the
 * ice model.  Filled by airice_atmosphere_* (readATMpar .cc:24-71, readnhFromFile
 * .cc:73-147, MakeAtmosphere .cc:920-942, FillInAirRefractiveIndex .cc:193-213). */
typedef struct airice_medium {
  double atmlay_cm[5];   /* ATMLAY (cm); [4] forced to 1.5e7 (.cc:66) */
  double abc[5][3];      /* mass-overburden a,b,c rows; abc[4]=abc[3] (.cc:62-64) */
  double B_air[5];       /* n(h) = A_air + B_air[l]*exp(-C_air[l]*h) */
  double C_air[5];
  double N0;             /* natural cubic spline of n(h) at h=0 (.cc:203) */
  int32_t max_layers;    /* MaxLayers (.cc:142) */
  int32_t n_points;      /* knots in the flattened profile */
  double A_air;          /* 1.0 (.h:99) */
  double A_ice, B_ice, C_ice; /* 1.78, -0.43, 0.0132 (.h:64-66) */
  double pi;             /* variant constant */
  double h_top;          /* h_data.back().back(): last tabulated height, m (the Tx clamp of
                            SingleRayAirIceRefraction.C:40-45) */
  int32_t constant_air_index; /* pythonwrapper AirIceRayTracing::UseConstantRefractiveIndex
                                 (.h:54, default 0): honoured by AIRICE_VARIANT_PYWRAPPER only --
                                 GetB_air = 0, GetC_air = 1e-9, Getnz_air = A_const (.cc:173-238)
                                 and the launch bracket [90, thR] without the probe (.cc:955-982) */
  int32_t reserved_;
  double A_const;        /* pythonwrapper .h:72 (1.00) */
} airice_medium;

/* MakeRayTracingTable grid (.cc:12-21 globals, .cc:2019-2061 set-up). */
typedef struct airice_grid {
  double start_height;   /* LoopStartHeight, m (100000, .cc:2044) */
  double stop_height;    /* LoopStopHeight, m: ice, or ice+depth when Rx is in air */
  double height_step;    /* HeightStepSize, m (10) */
  int32_t height_steps;  /* TotalHeightSteps */
  double start_angle;    /* LoopStartAngle, deg (90.1) */
  double stop_angle;     /* LoopStopAngle, deg (180) */
  double angle_step;     /* AngleStepSize, deg (0.1) */
  int32_t angle_steps;   /* TotalAngleSteps */
  double depth_m;        /* AntennaDepth, m (negative = in ice) */
  double ice_m;          /* IceLayerHeight, m */
  int32_t in_ice;        /* AntennaDepth < 0 */
  int32_t table_rows;    /* rows the table holds: the reference skips every row whose Tx height
                            start_height - height_step*row is not > 0 (.cc:2082), a suffix of the
                            height_steps rows, so the table is table_rows x angle_steps entries
                            (height_steps itself stays TotalHeightSteps, which the lookup reads) */
} airice_grid;

#define AIRICE_TABLE_COLUMNS 11 /* float columns of AllTableAllAntData (.cc:2101-2111) */
#define AIRICE_RAY_FIELDS 18    /* GetRayTracingSolutions dummy[0..17] (.cc:1999-2016) */
#define AIRICE_SOLVE_FIELDS 17  /* Air2IceRayTracing dummy[0..16] (.cc:1597-1614) */
#define AIRICE_PYSOLVE_FIELDS 15 /* AirIceRayTracing::Air2IceRayTracing dummy[0..14] (pythonwrapper .cc:1070-1084) */
#define AIRICE_HDTIP_FIELDS 9   /* GetHorizontalDistanceToIntersectionPoint outputs (.cc:963-972) */

const char *airice_last_error(void);
const char *airice_version(void);

/* --- medium (host) ------------------------------------------------------ */
/* Parse a GDAS Atmosphere.dat from a file (replaces MakeAtmosphere(), .cc:920). */
int airice_atmosphere_load(const char *path, int variant, airice_medium *out);
/* Parse from an in-memory text image of the same file. */
int airice_atmosphere_parse(const char *text, size_t len, int variant, airice_medium *out);
/* n(z) of the medium (Getnz_air .cc:259, Getnz_ice .cc:188), host side. */
double airice_nz_air(const airice_medium *m, double z);
double airice_nz_ice(const airice_medium *m, double z);

/* --- table (MakeRayTracingTable) ---------------------------------------- */
/* Grid set-up exactly as .cc:2019-2061 (depth/ice in cm as the reference takes them). */
int airice_grid_init(airice_grid *g, double antenna_depth_cm, double ice_height_cm,
                     double height_step_m, double start_angle_deg, double stop_angle_deg,
                     double angle_step_deg);
/* Trace rows [row_begin, row_begin+row_count) x all angles of the grid (rows at or past
 * table_rows are skipped, as the reference skips Tx heights <= 0).
 * d_table: 11 float columns, column c of ray r at d_table[c*ld + r - row_begin*angle_steps]
 * (the AllTableAllAntData[ant][c][r] layout).  d_full (nullable): 18 double columns,
 * same indexing (GetRayTracingSolutions dummy[] for parity checks). */
int airice_table_launch(const airice_medium *m, const airice_grid *g, int32_t row_begin,
                        int32_t row_count, float *d_table, double *d_full, size_t ld,
                        void *stream);
/* Several antennas' tables in ONE launch (one grid over every antenna's rows; the reference's
 * per-antenna loop RunMultiRayCode.C:29-52 calls MakeRayTracingTable once per antenna): grids[a]
 * from airice_grid_init for antenna a (same angle grid for all), d_tables[a] its 11 float columns
 * with column stride lds[a] >= grids[a].table_rows * angle_steps.  Bit-identical to one
 * airice_table_launch per antenna; at most 32 antennas. */
int airice_table_launch_multi(const airice_medium *m, const airice_grid *grids, int32_t n_grids,
                              float *const *d_tables, const size_t *lds, void *stream);
int airice_table_host(const airice_medium *m, const airice_grid *g, int32_t row_begin,
                      int32_t row_count, float *h_table, double *h_full, size_t ld);

/* --- single forward ray (GetRayTracingSolutions) on the device ---------- */
/* n rays with per-ray (launch_deg, txh_m); ice/depth/in_ice uniform; out: 18 double columns. */
int airice_rays_launch(const airice_medium *m, const double *d_launch_deg, const double *d_txh,
                       double ice_h_m, double depth_m, int32_t in_ice, size_t n, double *d_out,
                       size_t ld, void *stream);

/* The same rays on the host (CPU), from the same source as the device kernels with the host's
 * correctly rounded sqrt and quotients (within ~1 ulp of the device's): the one-query
 * GetRayTracingSolutions of the C++ drop-in runs here, ~1 us against a ~10 us kernel round trip.
 * Host arrays; out: 18 double columns, stride ld. */
int airice_rays_host(const airice_medium *m, const double *launch_deg, const double *txh,
                     double ice_h_m, double depth_m, int32_t in_ice, size_t n, double *out,
                     size_t ld);

/* --- two-layer (double-exponential) firn ---------------------------------- */
/* The reference's second ice model (TransitionBoundary != 0, GetB_ice / GetC_ice .cc:150-185, the
 * two-layer ice leg of GetRayTracingSolutions .cc:1923-1990), as the physical piecewise profile:
 * the lower layer's B and C at both ends of the lower segment, the sine stepping by
 * n_up(b) / n_low(b) across the boundary (DESIGN.md §14 for the difference from the reference).
 * The *_firn entry points take the arguments of their namesakes plus the firn after the medium,
 * with the same output layouts and stream semantics; they use m->A_ice and ignore m->B_ice and
 * m->C_ice.  An antenna at or above the boundary (|depth| <= boundary_m) or in the air gives the
 * bits of the one-layer call with (A_ice, B[0], C[0]).  A NULL firn, a non-finite field,
 * boundary_m <= 0 or C[l] <= 0 returns AIRICE_EINVAL and writes nothing.
 * Known limit: the minimizer is one-layer.  airice_solve_*, airice_hdtip_* have no firn form, and a
 * lookup (airice_lookup_*) of a layered table reads the table correctly but answers its lanes
 * flagged AIRICE_LOOKUP_FALLBACK in the one-layer model of m: treat those lanes as unanswered.
 * airice_table_save does not record the firn: do not save a layered table yet. */
typedef struct airice_firn {   /* n(z) = m->A_ice + B[l] exp(-C[l] z), z >= 0 the depth in m; */
  double boundary_m;           /* l = 0 for z <= boundary_m, l = 1 below; > 0 and finite        */
  double B[2], C[2];           /* finite, C > 0                                                  */
} airice_firn;
#define AIRICE_FIRN_SUMMIT {14.9, {-0.5019, -0.448023}, {0.03247, 0.02469}}  /* with A_ice = 1.775 */
double airice_nz_firn(const airice_medium *m, const airice_firn *f, double z);
int airice_table_launch_firn(const airice_medium *m, const airice_firn *f, const airice_grid *g,
                             int32_t row_begin, int32_t row_count, float *d_table, double *d_full,
                             size_t ld, void *stream);
int airice_table_launch_multi_firn(const airice_medium *m, const airice_firn *f,
                                   const airice_grid *grids, int32_t n_grids,
                                   float *const *d_tables, const size_t *lds, void *stream);
int airice_table_host_firn(const airice_medium *m, const airice_firn *f, const airice_grid *g,
                           int32_t row_begin, int32_t row_count, float *h_table, double *h_full,
                           size_t ld);
int airice_rays_launch_firn(const airice_medium *m, const airice_firn *f,
                            const double *d_launch_deg, const double *d_txh, double ice_h_m,
                            double depth_m, int32_t in_ice, size_t n, double *d_out, size_t ld,
                            void *stream);
int airice_rays_host_firn(const airice_medium *m, const airice_firn *f, const double *launch_deg,
                          const double *txh, double ice_h_m, double depth_m, int32_t in_ice,
                          size_t n, double *out, size_t ld);

/* Where one-query calls run: AIRICE_SCALAR_HOST (default: the calling CPU thread, from the same
 * __host__ __device__ source as the kernels, with the host's correctly rounded sqrt and quotients,
 * so within about an ulp of the same query inside a GPU batch) or AIRICE_SCALAR_DEVICE (a
 * one-wave GPU kernel per call, bit-identical to the batch).  The mode covers every one-query
 * call: GetRayTracingSolutions and the ray layer of the C++ drop-ins (airice_rtf_eval / _variant:
 * RayTracingFunctions::, MultiRayAirIceRefraction:: and AirIceRayTracing:: fDnfR ...
 * MinimizeforLaunchAngle), the one-query solves (Air2IceRayTracing, the CoREAS entry,
 * Py_TraceIceToAir, the _Table lookup's minimizer fallback) and airice_solve_host /
 * airice_trace_ice_to_air_host calls with n == 1.  The environment variable AIRICE_SCALAR=device
 * selects the device at start.  Returns the previous mode; any other value only queries it.
 * Batch entry points (n > 1 and every *_launch) always run on the GPU; airice_rays_host always
 * runs on the host. */
#define AIRICE_SCALAR_HOST 0
#define AIRICE_SCALAR_DEVICE 1
int airice_scalar_mode(int mode);

/* --- minimizer (Air2IceRayTracing) --------------------------------------- */
/* Batched launch-angle solve.  Inputs in metres: Tx height, horizontal distance, Rx
 * depth (negative = below the ice surface); ice height uniform.  d_straight_angle is
 * Air2IceRayTracing's StraightAngle argument (.cc:1464) in degrees; when NULL it is
 * formed per query as GetHorizontalDistanceToIntersectionPoint does (.cc:952-958).
 * d_out: AIRICE_SOLVE_FIELDS (MultiRay) or AIRICE_PYSOLVE_FIELDS (pythonwrapper)
 * double columns, stride ld.  d_status (nullable): AIRICE_SOLVE_* bits.
 * airice_solve_host is the same with every array on the host; with ld > n it writes entries
 * [0, n) of each column only: the padding out[c*ld + n .. c*ld + ld) is left as the caller had
 * it (earlier builds of the library overwrote it with undefined values).  n == 1 runs where
 * airice_scalar_mode says: on the calling thread, or on the device through the scalar slot as
 * every other one-query call does (earlier builds took the batch route's device block for it; the
 * kernel and the bits are the same).  The same holds for airice_trace_ice_to_air_host. */
int airice_solve_launch(const airice_medium *m, int variant, double ice_h_m,
                        const double *d_txh, const double *d_dist, const double *d_depth,
                        const double *d_straight_angle, size_t n, double *d_out, size_t ld,
                        uint8_t *d_status, void *stream);
int airice_solve_host(const airice_medium *m, int variant, double ice_h_m, const double *txh,
                      const double *dist, const double *depth, const double *straight_angle,
                      size_t n, double *out, size_t ld, uint8_t *status);

/* CoREAS entry, batched: GetHorizontalDistanceToIntersectionPoint (.cc:945-989) with cm
 * inputs; d_out: 9 double columns (opticalPathLengthInIce, opticalPathLengthInAir,
 * geometricalPathLengthInIce, geometricalPathLengthInAir, launchAngle [rad],
 * horizontalDistanceToIntersectionPoint, transmissionCoefficientS,
 * transmissionCoefficientP, RecievedAngleInIce [rad]); d_ok: the returned bool. */
int airice_hdtip_launch(const airice_medium *m, const double *d_src_cm, const double *d_dist_cm,
                        const double *d_depth_cm, double ice_cm, size_t n, double *d_out,
                        size_t ld, uint8_t *d_ok, void *stream);

/* --- table lookup (GetHorizontalDistanceToIntersectionPoint_Table) -------- */
/* One antenna's table resident in HBM (the AllTableAllAntData[ant] a MakeRayTracingTable /
 * airice_table_launch produced) plus the grid globals the reference reads at lookup time
 * (LoopStopHeight, HeightStepSize, TotalHeightSteps, TotalAngleSteps of the LAST table made,
 * .cc:1035-1039). */
typedef struct airice_lookup_table {
  const float *table;         /* device: column c of entry i at table[c*ld + i] */
  size_t ld;                  /* column stride in floats */
  size_t n_entries;           /* AllTableAllAntData[ant][0].size() */
  double loop_stop_height;    /* m */
  double height_step;         /* m */
  int32_t total_height_steps;
  int32_t total_angle_steps;
  const float *entries;       /* optional device copy from airice_lookup_pack (NULL: the lookup
                                 reads the columns only); same values, fewer cache lines */
} airice_lookup_table;

/* The packed copy (pack format 2, library 0.2; format 1 of 0.1.x had 32-float pair records and
 * no angle vector -- a buffer sized for it is too small and airice_lookup_pack refuses it):
 *  - pair records: record i holds columns 2, 3, 5, 6, 7, 8, 9, 10 of entry i (floats 0-7) and of
 *    entry i + 1 (floats 8-15; NaN for the last entry): 64 B, one fabric request when the array
 *    is 64-byte aligned.  The lookup interpolates between entries i and i + 1 (FindClosestTHD's
 *    index1, index2), so each table row it visits costs it one record; the THD values at the pair
 *    (column 1) come from its own search, the launch angles (column 4) from the angle vector;
 *  - row records, from float AIRICE_LOOKUP_ROWS_OFFSET(n_entries) on (128-byte aligned), one per
 *    full table row (n_entries / total_angle_steps rows): the row's FindClosestAirTxHeight span,
 *    the table values the lookup reads at its ends and the THD values of the first four
 *    FindClosestTHD bisection steps on both interpolation heights' spans (two 128-byte lines);
 *  - the angle vector: column 4 of the first row (total_angle_steps floats, padded to 4), then one
 *    int32 word: 1 when every row's column 4 equals it bit for bit (a MakeRayTracingTable table:
 *    the launch angle is the grid's, .cc:2084-2105), else 0 and the lookup reads column 4. */
#define AIRICE_LOOKUP_ENTRY_FLOATS 16
#define AIRICE_LOOKUP_ROW_FLOATS 64
#define AIRICE_LOOKUP_ROWS_OFFSET(n_entries) \
  (((size_t)(n_entries) * AIRICE_LOOKUP_ENTRY_FLOATS + 31) / 32 * 32)
/* Floats of the whole packed copy. */
#define AIRICE_LOOKUP_PACK_FLOATS(n_entries, angle_steps)                          \
  (AIRICE_LOOKUP_ROWS_OFFSET(n_entries) +                                         \
   ((size_t)(n_entries) / (size_t)(angle_steps)) * AIRICE_LOOKUP_ROW_FLOATS +     \
   ((size_t)(angle_steps) + 3) / 4 * 4 + 4)
/* The same, as a call (0 when n_entries or total_angle_steps is < 1). */
size_t airice_lookup_pack_floats(size_t n_entries, int32_t total_angle_steps);

/* Pack one antenna's table for the lookup into d_entries: capacity_floats (at least
 * AIRICE_LOOKUP_PACK_FLOATS(n_entries, total_angle_steps), else AIRICE_EINVAL and nothing is
 * written) device floats, 16-byte aligned (64-byte for one request per pair record).  The lookup
 * then reads the interpolated parameters of both entries of a pair from one record instead of 10
 * columns ld floats apart; results are identical.  Stream-ordered; run once per table, then set
 * t->entries = d_entries. */
int airice_lookup_pack(const airice_lookup_table *t, float *d_entries, size_t capacity_floats,
                       void *stream);

#define AIRICE_LOOKUP_FALLBACK 1 /* the minimizer fallback ran (.cc:1418-1420) */
#define AIRICE_LOOKUP_UNPINNED 2 /* the reference reads uninitialised/out-of-range memory here:
                                    such slots are returned as 0 / NaN */

/* Batched GetHorizontalDistanceToIntersectionPoint_Table (.cc:1305-1462) for one antenna
 * (AntennaNumber already resolved by the caller, .cc:1348-1352): cm inputs, ice height
 * uniform; d_out: the 9 double columns of airice_hdtip_launch, d_ok: the returned bool,
 * d_flags (required): AIRICE_LOOKUP_* bits.  Lanes hitting the reference's one-sided
 * extrapolation case run its minimizer fallback on the device, with the reference's
 * argument handling (cm values scaled by 100 once more, optical/geometric slots swapped). */
int airice_table_lookup_launch(const airice_medium *m, const airice_lookup_table *t,
                               const double *d_src_cm, const double *d_dist_cm,
                               const double *d_depth_cm, double ice_cm, size_t n,
                               double *d_out, size_t ld, uint8_t *d_ok, uint8_t *d_flags,
                               void *stream);

#define AIRICE_LOOKUP_MAX_TABLES 32
/* Batched _Table for n_ant antennas x n_src sources in ONE launch (lookup_multi_kernel).  Query
 * (a, i): source height d_src_cm[i], distance d_dist_cm[a*ld_dist + i], Rx depth
 * antenna_depth_cm[a], table tables[antenna_table[a]] (antennas at one depth share a table,
 * .cc:1348-1352).  Column c of query (a, i) at d_out[c*ld + a*n_src + i]; d_ok / d_flags at
 * [a*n_src + i].  Bit-identical (outputs, ok, flags) to one airice_table_lookup_launch per antenna.
 * The source heights are common to all antennas, so a caller that sorts them once (and permutes
 * the distance rows alike) gives every antenna the faster sorted order.
 * tables (1..AIRICE_LOOKUP_MAX_TABLES of them, packed or not, each with its own grid globals),
 * antenna_table and antenna_depth_cm (n_ant each): host arrays, read before the call returns.
 * d_work: work_bytes >= airice_table_lookup_multi_work_bytes(n_tables, n_ant) device bytes, 16-byte
 * aligned; the launch uploads the table descriptions and the antenna records into it.
 * Stream-ordered, no device allocation (the upload reads the host arrays during the call, so the
 * call is not one to capture into a graph).  An argument airice_table_lookup_launch would refuse
 * (checked per table), n_tables outside 1..32, antenna_table[a] outside [0, n_tables),
 * ld_dist < n_src, ld < n_ant*n_src, n_src >= 2^32 or a workspace that is too small is
 * AIRICE_EINVAL before any device call (airice_last_error() names the offending index);
 * n_ant == 0 or n_src == 0 is AIRICE_OK and nothing is launched. */
size_t airice_table_lookup_multi_work_bytes(int32_t n_tables, int32_t n_ant);
int airice_table_lookup_launch_multi(const airice_medium *m, const airice_lookup_table *tables,
                                     int32_t n_tables, const int32_t *antenna_table,
                                     const double *antenna_depth_cm, int32_t n_ant,
                                     const double *d_src_cm, const double *d_dist_cm,
                                     size_t ld_dist, double ice_cm, size_t n_src, double *d_out,
                                     size_t ld, uint8_t *d_ok, uint8_t *d_flags, void *d_work,
                                     size_t work_bytes, void *stream);

/* --- single ray + path sampler (SingleRayAirIceRefraction, BASELINE cfg1) ---------------- */
/* SingleRayAirIceRefraction.C:33-299 over RayTracingFunctions.cc: inputs are the CLI's values
 * after its clamps (Tx <= h_top, launch > 90, .C:40-51), metres/degrees, antenna depth
 * POSITIVE below the ice surface (.C:166).  Path samples are the lines of
 * RayPathinAirnIce.txt in order: x (m) and height z (m). */
typedef struct airice_single_ray_info {
  int32_t skip_above, skip_below; /* SkipLayersAbove / SkipLayersBelow (.C:60-86) */
  int32_t n_layers;               /* MaxLayers - SkipLayersAbove - SkipLayersBelow (.C:226) */
  int32_t pad_;
  int64_t n_air, n_ice;           /* path samples in air (.C:247) and ice (.C:292) */
} airice_single_ray_info;
/* summary: total horizontal distance in air (.C:157), L, incident angle on the ice (deg),
 * horizontal distance / receive angle (deg) / propagation time (s) in ice (.C:167-170) */
#define AIRICE_SINGLE_RAY_FIELDS 6
#define AIRICE_SINGLE_RAY_WORK 32 /* doubles of d_summary: the summary, then sampler constants */
int airice_single_ray_plan(const airice_medium *m, double antenna_depth_m, double launch_deg,
                           double txh_m, double ice_m, airice_single_ray_info *info);
/* d_summary: AIRICE_SINGLE_RAY_WORK doubles (summary in the first AIRICE_SINGLE_RAY_FIELDS);
 * d_x/d_z (nullable together): cap >= n_air + n_ice */
int airice_single_ray_launch(const airice_medium *m, double antenna_depth_m, double launch_deg,
                             double txh_m, double ice_m, double *d_summary, double *d_x,
                             double *d_z, size_t cap, void *stream);
int airice_single_ray_host(const airice_medium *m, double antenna_depth_m, double launch_deg,
                           double txh_m, double ice_m, double *summary, double *x, double *z,
                           size_t cap);

/* --- ray paths of many rays in one launch (the per-point loop of DrawShowerRays.C:483-519) --- */
/* n rays that share the ice height and the antenna depth (positive in ice), each with its own
 * launch angle and Tx height; ray i is exactly what airice_single_ray_* gives for
 * (antenna_depth_m, launch_deg[i], txh_m[i], ice_m): the same six summary values, the same
 * n_air + n_ice samples in RayPathinAirnIce.txt order, the same bits (both paths run the same
 * device functions).
 *
 * Plan (host only, no GPU needed): offsets[0..n], offsets[0] = 0; ray i owns samples
 * [offsets[i], offsets[i+1]) of x and z.  The count depends on (txh, ice, depth) only, not on the
 * launch angle.  *work_bytes (nullable): the size of the launch's workspace.  A ray that
 * airice_single_ray_plan rejects fails the batch with AIRICE_EINVAL; airice_last_error() names
 * its index. */
int airice_ray_paths_plan(const airice_medium *m, double antenna_depth_m, double ice_m,
                          const double *txh_m /* host */, size_t n, int64_t *offsets /* host, n+1 */,
                          size_t *work_bytes);
/* Stream-ordered, no device allocation: two kernels (ray_consts_kernel: one lane per ray;
 * ray_paths_kernel: one lane per sample of the whole batch) after the upload of the per-ray plans
 * into d_work.  d_launch_deg: n device doubles (for instance column 10, LaunchAngleAir, of an
 * airice_solve_launch output); txh_m and offsets: host, as given to / filled by the plan (checked
 * against it); d_work: work_bytes device bytes, 16-byte aligned; d_summary: the six
 * airice_single_ray summary values as double columns, value f of ray i at d_summary[f*ld + i];
 * d_x / d_z (nullable together: summaries only): cap >= offsets[n] doubles each.  A cap or
 * work_bytes that is too small is AIRICE_EINVAL and nothing is launched; n == 0 is AIRICE_OK and
 * nothing is launched. */
int airice_ray_paths_launch(const airice_medium *m, double antenna_depth_m, double ice_m,
                            const double *d_launch_deg, const double *txh_m, size_t n,
                            const int64_t *offsets, void *d_work, size_t work_bytes,
                            double *d_summary, size_t ld, double *d_x, double *d_z, size_t cap,
                            void *stream);
/* The same with every array on the host (summary: 6 columns of stride ld; x / z nullable
 * together): copies, launches and synchronises. */
int airice_ray_paths_host(const airice_medium *m, double antenna_depth_m, double ice_m,
                          const double *launch_deg, const double *txh_m, size_t n,
                          const int64_t *offsets, double *summary, size_t ld, double *x, double *z,
                          size_t cap);

/* pythonwrapper TraceIceToAir, batched: per-query (depth, ice, txh, dist) metres ->
 * ArrayParameters[10] rows (TraceIceToAir.C:46-68), row-major n x 10. */
int airice_trace_ice_to_air_launch(const airice_medium *m, const double *d_depth,
                                   const double *d_ice, const double *d_txh,
                                   const double *d_dist, size_t n, double *d_out10,
                                   void *stream);
int airice_trace_ice_to_air_host(const airice_medium *m, const double *depth, const double *ice,
                                 const double *txh, const double *dist, size_t n, double *out10);

/* Drop-in for the reference ctypes symbol (TraceIceToAir.C:75-79): the C++ TraceIceToAir of
 * include/AirIceRayTracing.h, which reads "Atmosphere.dat" from the working directory like the
 * reference (parsed once while the file is unchanged; falls back to $AIRICE_ATMOSPHERE), then
 * solves the one query where airice_scalar_mode says: the calling thread by default, a one-wave
 * GPU kernel with AIRICE_SCALAR=device.  Batches: airice_trace_ice_to_air_launch. */
void Py_TraceIceToAir(double AntennaDepth, double IceLayerHeight, double AirTxHeight,
                      double HorizontalDistance, double ArrayParameters[10]);

/* --- RayTracingFunctions:: scalar layer (RayTracingFunctions.cc, the cfg1 CLI's library) --- */
/* One call evaluated with the reference's expressions (pi 3.1415927) on the host, or on the
 * device (airice_scalar_mode); host arguments and outputs, synchronous.  For the
 * RayTracingFunctions.h drop-in (include/RayTracingFunctions.h); batches belong on the table /
 * solve / single-ray paths. */
#define AIRICE_RTF_HIT_POINT 0        /* GetLayerHitPointPar (.cc:399-527)
                                         args {n_layer1, RxDepth, TxDepth, IncidentAng, AirOrIce}
                                         -> {THD, ReceiveAngle deg, L, time s} */
#define AIRICE_RTF_OPTICAL_PATH 1     /* GetRayOpticalPath (.cc:349-369)
                                         args {A, RxDepth, TxDepth, Lvalue, AirOrIce} -> {x} */
#define AIRICE_RTF_PROPAGATION_TIME 2 /* GetRayPropagationTime (.cc:371-397), args as above */
#define AIRICE_RTF_AIR_PROPAGATION 3  /* GetAirPropagationPar (.cc:529-659)
                                         args {LaunchAngle, AirTxHeight, IceLayerHeight}
                                         -> 4 x MaxLayers {THD, Recv, L, t} + count */
#define AIRICE_RTF_ICE_PROPAGATION 4  /* GetIcePropagationPar (.cc:661-681) args {IncidentAngle,
                                         IceLayerHeight, AntennaDepth, Lvalue} -> {THD, Recv, L, t} */
#define AIRICE_RTF_FDNFR 5            /* fDnfR (.cc:293-303) args {x, a, b, c, l} -> {value} */
#define AIRICE_RTF_FTIMED 6           /* ftimeD (.cc:328-347) args {x, a, b, c, speedc, l,
                                         airorice} -> {value} */
#define AIRICE_RTF_MIN_LAUNCH 7       /* MinimizeforLaunchAngle (.cc:683-731) args {x, airtxheight,
                                         icelayerheight, antennadepth, horizontaldistance} */
#define AIRICE_RTF_AIR2ICE 8          /* the Air2IceRayTracing CLI's solve (Air2IceRayTracing.C:56-185):
                                         args {AirTxHeight, HorizontalDistance, IceLayerHeight,
                                         AntennaDepth (> 0 in ice)} -> AIRICE_RTF_AIR2ICE_FIELDS:
                                         launch-angle bracket and its probe, GSL-Brent root of
                                         MinimizeforLaunchAngle (FindFunctionRoot, .cc:256-290,
                                         max_iter 20, tolerance 1e-9), air and ice results */
#define AIRICE_RTF_AIR2ICE_FIELDS 16  /* {startangle, endangle, LaunchAngleAir, THD_air,
                                         IncidentAngleonIce, Lvalue, t_air ns, THD_ice,
                                         IncidentAngleonAntenna, t_ice ns, THD, t ns,
                                         status (AIRICE_SOLVE_* bits), Brent iterations,
                                         probe steps, filled air layers} */
/* MultiRayAirIceRefraction:: forms of the same layer (MultiRayAirIceRefraction.cc:377-917, the
 * MultiRayAirIceRefraction.h drop-in): 5-wide outputs {THD, ReceiveAngle deg, L, time s,
 * geometric path}.  fDnfR, ftimeD and GetRayPropagationTime are the AIRICE_RTF_ ops above
 * (identical expressions), GetRayHorizontalPath is AIRICE_RTF_OPTICAL_PATH. */
#define AIRICE_MR_FPATHD 9            /* fpathD (.cc:434-447) args {x, a, b, c, speedc, l} */
#define AIRICE_MR_GEOMETRIC_PATH 10   /* GetRayGeometricPath (.cc:494-513)
                                         args {A, RxDepth, TxDepth, Lvalue, AirOrIce} */
#define AIRICE_MR_HIT_POINT 11        /* GetLayerHitPointPar (.cc:521-646)
                                         args {n_layer1, RxDepth, TxDepth, IncidentAng, AirOrIce} */
#define AIRICE_MR_AIR_PROPAGATION 12  /* GetAirPropagationPar (.cc:661-804) args {LaunchAngle,
                                         AirTxHeight, IceLayerHeight} -> 5 x MaxLayers + 2,
                                         filled-layer count at [5*MaxLayers+1] */
#define AIRICE_MR_ICE_PROPAGATION 13  /* GetIcePropagationPar (.cc:807-869) args {IncidentAngleonIce,
                                         IceLayerHeight, AntennaDepth, Lvalue} -> 5 */
#define AIRICE_MR_MIN_LAUNCH 14       /* MinimizeforLaunchAngle (.cc:873-917) args {x, airtxheight,
                                         icelayerheight, antennadepth, horizontaldistance} */
/* Outputs written for op (4 x max_layers + 1 for AIR_PROPAGATION, 5 x max_layers + 2 for
 * MR_AIR_PROPAGATION), or -1 for an unknown op. */
int airice_rtf_outputs(int op, int max_layers);
int airice_rtf_eval(const airice_medium *m, int op, const double *args, size_t n_args,
                    double *out, size_t n_out);
/* The same ops with the numerics of another reference namespace: AIRICE_VARIANT_PYWRAPPER gives the
 * pythonwrapper's AirIceRayTracing:: ray layer (pythonwrapper/AirIceRayTracing.cc:356-857, the
 * AIRICE_MR_* / FDNFR / FTIMED / OPTICAL_PATH / PROPAGATION_TIME ops with pi = 4*atan(1) and its
 * UseConstantRefractiveIndex medium); airice_rtf_eval is AIRICE_VARIANT_MULTIRAY. */
int airice_rtf_eval_variant(const airice_medium *m, int variant, int op, const double *args,
                            size_t n_args, double *out, size_t n_out);

/* AIRICE_RTF_AIR2ICE for a batch: the point-to-point solve of the stand-alone programs
 * Air2IceRayTracing.C:56-185 and AirRayTracing.C (launch-angle bracket and probe, GSL Brent under
 * FindFunctionRoot, the air and ice legs at the root) for n transmitter/receiver pairs in ONE
 * launch of air2ice_kernel, one pair per lane.  Per pair: Tx height, horizontal distance, ice
 * height and antenna depth (m, depth > 0 in ice), so an air-to-air pair is
 * (max(Tx, Rx), D, min(Tx, Rx), 0) (AirRayTracing.C:38-45, its receive angle reported as
 * 180 - angle when the two were swapped) and mixes freely with air-to-ice pairs.  Value c of pair
 * i (the AIRICE_RTF_AIR2ICE_FIELDS above) lands at d_out[c*ld + i]; d_status (nullable): value 12,
 * the AIRICE_SOLVE_* bits, as a byte.  Column 2 (d_out + 2*ld) is a contiguous d_launch_deg for
 * airice_ray_paths_launch.  The bits are those of airice_rtf_eval(AIRICE_RTF_AIR2ICE) on the
 * device for each pair alone (the search reads only the summed distance and L of each trial angle,
 * accumulated in the same order), so they do not depend on the batch or its order.  Every pair
 * terminates, non-finite inputs included (at most 1,779 probe steps and 20 Brent iterations).
 * Stream-ordered, no device allocation, exactly one kernel launch; n == 0 is AIRICE_OK and nothing
 * is launched; a null required pointer or ld < n is AIRICE_EINVAL before any device call, and
 * airice_last_error() names the argument. */
int airice_air2ice_launch(const airice_medium *m, const double *d_txh, const double *d_dist,
                          const double *d_ice, const double *d_depth, size_t n, double *d_out,
                          size_t ld, uint8_t *d_status, void *stream);
/* The same with every array on the host: n == 1 runs where airice_scalar_mode says (the calling
 * thread, or the kernel through the one-query slot); n > 1 copies, launches and synchronises. */
int airice_air2ice_host(const airice_medium *m, const double *txh, const double *dist,
                        const double *ice, const double *depth, size_t n, double *out, size_t ld,
                        uint8_t *status);

/* --- in-ice rays (IceRayTracing::IceRayTracing, IceRayTracing.cc:1745-1919) ---------------------
 * The direct, reflected and refracted rays between a transmitter at (0, z0) and a receiver at
 * (x1, z1), both in the ice (depths negative, metres), for n pairs in ONE launch of iceray_kernel,
 * one pair per lane: GetDirectRayPar, GetReflectedRayPar and -- when either failed --
 * GetRefractedRayPar, with the reference's false-position and Newton searches (GSL semantics
 * restated) and every acceptance decision as written.  Three deliberate departures (DESIGN.md
 * §8): the turning depth is the closed form ln(B/(L-A))/C, the receive / incidence angles are
 * asin(L/n(z)), and the index just below a turning depth is formed without cancellation.  model3 = {A, B, C} of n(z) = A + B exp(-C|z|) on the HOST in both entry points
 * (SetA / SetB / SetC); NULL is 1.78, -0.43, 0.0132.
 * Value c of pair i lands at d_out[c*ld + i]; columns 0..28 are the reference's output[0..28]:
 *   0-3 launch angle (deg) of D, R, Ra0, Ra1; 4-7 their times (s); 8-11 their receive angles
 *   (-1000: no such ray); 12-13, 14-15, 16-17 the two legs' times of R, Ra0, Ra1 (0.0 when the
 *   ray failed; uninitialised in the reference); 18 incidence angle at the surface; 19-22 the L
 *   parameters; 23-24 turning depths of Ra0, Ra1; 25-28 geometric paths (m).
 *   29 status byte as a double, 30 residual evaluations, 31 false-position iterations of the
 *   direct search.
 * Status (also d_status, nullable): AIRICE_ICERAY_D / _R / _RA0 / _RA1 set when that ray is
 * accepted (|checkzero| < 0.5); AIRICE_ICERAY_NONFINITE alone for a NaN or infinite input, whose
 * columns 0..28 are NaN and for which no search runs.  Every pair terminates (each search is at
 * most 100 iterations, at most 9 searches per pair).  Pairs are independent: results do not depend
 * on the batch or its order.
 * Stream-ordered, no device allocation, exactly one kernel launch; n == 0 is AIRICE_OK and nothing
 * is launched; a null required pointer or ld < n is AIRICE_EINVAL before any device call, and
 * airice_last_error() names the argument. */
#define AIRICE_ICERAY_FIELDS 32
#define AIRICE_ICERAY_REFERENCE_FIELDS 29
#define AIRICE_ICERAY_LAUNCH_ANGLE 0
#define AIRICE_ICERAY_TIME 4
#define AIRICE_ICERAY_RECEIVE_ANGLE 8
#define AIRICE_ICERAY_LEG_TIMES 12
#define AIRICE_ICERAY_INCIDENCE 18
#define AIRICE_ICERAY_LVALUE 19
#define AIRICE_ICERAY_ZMAX 23
#define AIRICE_ICERAY_PATH 25
#define AIRICE_ICERAY_STATUS 29
#define AIRICE_ICERAY_EVALS 30
#define AIRICE_ICERAY_ITERS 31
#define AIRICE_ICERAY_D 1
#define AIRICE_ICERAY_R 2
#define AIRICE_ICERAY_RA0 4
#define AIRICE_ICERAY_RA1 8
#define AIRICE_ICERAY_NONFINITE 128
int airice_iceray_launch(const double *model3, const double *d_z0, const double *d_x1,
                         const double *d_z1, size_t n, double *d_out, size_t ld,
                         uint8_t *d_status, void *stream);
/* The same with every array on the host: n == 1 runs where airice_scalar_mode says (the calling
 * thread, or the kernel through the one-query slot); n > 1 copies, launches and synchronises. */
int airice_iceray_host(const double *model3, const double *z0, const double *x1, const double *z1,
                       size_t n, double *out, size_t ld, uint8_t *status);

/* --- ice-to-air direct ray (IceRayTracing::GetDirectRayPar_Air, IceRayTracing.cc:2358-2500) ------
 * The direct ray from a transmitter at depth d_z0 (<= 0) in the ice to a receiver d_x1 metres away
 * and d_h (> 0) metres ABOVE the surface -- refracting in the ice, straight in the air at n = 1 --
 * for n triples in ONE launch of iceair_kernel, one triple per lane: the reference's false
 * position of fDa_Air on [1e-7, min(n(1e-7), n(z0))] (GSL semantics restated, at most 100
 * iterations) and its closing arithmetic as written, with the receive angle in ice taken as
 * asin(L/n(1e-7)) and the air angle's tangent and cosine taken from its sine, L (DESIGN.md §8,
 * §13).  model3 as airice_iceray_launch.
 * Value c of triple i lands at d_out[c*ld + i]:
 *   0 receive angle in air, deg (-1000 when |checkzero| > 0.5); 1 launch angle, deg; 2 time, s, as
 *   the reference forms it -- its air leg is the HORIZONTAL distance over c; 3 L; 4 checkzero;
 *   5 status byte as a double; 6 residual evaluations; 7 false-position iterations;
 *   8 (extension) the physical time, ice time + h / (c cos(air angle)); 9 (extension) the
 *   geometric path, ice path + h / cos(air angle).
 * Status (also d_status, nullable): AIRICE_ICEAIR_ACCEPTED when |checkzero| <= 0.5;
 * AIRICE_ICEAIR_NONFINITE alone for a NaN or infinite input, whose columns 0-4 and 8-9 are NaN and
 * for which no search runs.  No other input is special: h <= 0 or z0 > 0 run the arithmetic as
 * written.  Triples are independent: results do not depend on the batch or its order.
 * Stream-ordered, no device allocation, exactly one kernel launch; n == 0 is AIRICE_OK and nothing
 * is launched; a null required pointer or ld < n is AIRICE_EINVAL before any device call, and
 * airice_last_error() names the argument. */
#define AIRICE_ICEAIR_FIELDS 10
#define AIRICE_ICEAIR_RECEIVE_ANGLE 0
#define AIRICE_ICEAIR_LAUNCH_ANGLE 1
#define AIRICE_ICEAIR_TIME 2
#define AIRICE_ICEAIR_LVALUE 3
#define AIRICE_ICEAIR_CHECKZERO 4
#define AIRICE_ICEAIR_STATUS 5
#define AIRICE_ICEAIR_EVALS 6
#define AIRICE_ICEAIR_ITERS 7
#define AIRICE_ICEAIR_PHYSICAL_TIME 8
#define AIRICE_ICEAIR_PATH 9
#define AIRICE_ICEAIR_ACCEPTED 1
#define AIRICE_ICEAIR_NONFINITE 128
int airice_iceair_launch(const double *model3, const double *d_z0, const double *d_x1,
                         const double *d_h, size_t n, double *d_out, size_t ld,
                         uint8_t *d_status, void *stream);
/* The same with every array on the host: n == 1 runs where airice_scalar_mode says (the calling
 * thread, or the kernel through the one-query slot); n > 1 copies, launches and synchronises. */
int airice_iceair_host(const double *model3, const double *z0, const double *x1, const double *h,
                       size_t n, double *out, size_t ld, uint8_t *status);

/* --- first arrivals between 3-D points (IceRayTracing::DirectRayTracer, IceRayTracing.cc:
 * 2502-2612) -------------------------------------------------------------------------------------
 * The first-arriving ray from each emitter (d_tx_x, d_tx_y, d_tx_z) to each antenna (d_rx_*), all
 * in the ice, in three launches behind this one entry: icefirst_geom_kernel forms
 * (z0, x1, z1) = (zT, sqrt(dx*dx + dy*dy), zR) per pair (no fused multiply-add, the correctly
 * rounded root), iceray_kernel solves them (airice_iceray_launch's kernel), and
 * icefirst_select_kernel makes the reference's choice: among D, Ra0 and Ra1 -- those whose receive
 * angle is not -1000; never the reflected ray -- the first whose time*c is strictly the smallest,
 * starting from min = 1e9.
 * pairing: AIRICE_PAIRS_ELEMENTWISE (n_tx == n_rx, pair i = emitter i, antenna i) or
 * AIRICE_PAIRS_CROSS (pair t*n_rx + r = emitter t, antenna r).  Every intermediate lives in
 * d_work, work_bytes >= airice_icefirst_work_bytes(pairs) bytes of device memory.
 * Value c of pair i lands at d_out[c*ld + i]: 0 launch angle, deg; 1 receive angle, deg;
 * 2 geometric path, m; 3 time*c, m; 4 time, s; 5 the ray, with airice_icesol's codes (1 D, 3 Ra0,
 * 4 Ra1; 0 none); 6 x1; 7 the solver's status byte (AIRICE_ICERAY_* bits; also d_status,
 * nullable).  With no candidate columns 0-4 are -1000; a non-finite coordinate gives NaN there,
 * ray 0 and AIRICE_ICERAY_NONFINITE.
 * Stream-ordered, no device allocation; zero pairs is AIRICE_OK and nothing is launched; an unknown
 * pairing, n_tx != n_rx with AIRICE_PAIRS_ELEMENTWISE, a null pointer, ld < pairs or a work_bytes
 * too small is AIRICE_EINVAL before any device call, and airice_last_error() names the argument. */
#define AIRICE_ICEFIRST_FIELDS 8
#define AIRICE_ICEFIRST_LAUNCH_ANGLE 0
#define AIRICE_ICEFIRST_RECEIVE_ANGLE 1
#define AIRICE_ICEFIRST_PATH 2
#define AIRICE_ICEFIRST_TIME_C 3
#define AIRICE_ICEFIRST_TIME 4
#define AIRICE_ICEFIRST_RAY_TYPE 5
#define AIRICE_ICEFIRST_X1 6
#define AIRICE_ICEFIRST_STATUS 7
#define AIRICE_PAIRS_ELEMENTWISE 0
#define AIRICE_PAIRS_CROSS 1
size_t airice_icefirst_work_bytes(size_t n_pairs);
int airice_icefirst_launch(const double *model3, const double *d_tx_x, const double *d_tx_y,
                           const double *d_tx_z, size_t n_tx, const double *d_rx_x,
                           const double *d_rx_y, const double *d_rx_z, size_t n_rx, int pairing,
                           void *d_work, size_t work_bytes, double *d_out, size_t ld,
                           uint8_t *d_status, void *stream);
/* The last of the three launches on its own, for a caller that holds the solver's rows already:
 * the choice over d_rays, the 32 columns airice_iceray_launch wrote (stride ld_rays), with d_x1
 * passed through to column 6.  ONE launch of icefirst_select_kernel, stream-ordered, no device
 * allocation; n == 0 is AIRICE_OK; a null d_rays, d_x1 or d_out, ld_rays < n or ld < n is
 * AIRICE_EINVAL before any device call. */
int airice_icefirst_select_launch(const double *d_rays, size_t ld_rays, const double *d_x1,
                                  size_t n, double *d_out, size_t ld, uint8_t *d_status,
                                  void *stream);
/* The same choice over host rows, on the calling thread; no GPU. */
int airice_icefirst_select_host(const double *rays, size_t ld_rays, const double *x1, size_t n,
                                double *out, size_t ld, uint8_t *status);
/* The same with every array on the host and no work buffer: one pair runs where airice_scalar_mode
 * says (the calling thread, or the three kernels through the one-query slot); more are copied,
 * launched and synchronised. */
int airice_icefirst_host(const double *model3, const double *tx_x, const double *tx_y,
                         const double *tx_z, size_t n_tx, const double *rx_x, const double *rx_y,
                         const double *rx_z, size_t n_rx, int pairing, double *out, size_t ld,
                         uint8_t *status);

/* --- the two rays a receiver sees (IceRayTracing::GetRayTracingSolutions, IceRayTracing.cc:
 * 2907-3210) and their focusing factors (GetFocusingFactor, .cc:3218-3293) ----------------------
 * For n pairs in ONE launch of icesol_kernel, one pair per lane, over the rows airice_iceray_launch
 * wrote: d_rays (32 columns of stride ld_rays) for (d_z0, d_x1, d_z1) and -- nullable; NULL means
 * no focusing -- d_rays_lower (stride ld_lower) for (d_z0, d_x1, d_z1 - 0.01).  The choice of the
 * two rays, IgnoreCh, the swap by arrival time and the straight-line rule for equal depths are
 * the reference's statements as written; the ice attenuation along each chosen ray is
 * AttRay = 1 - a0 * integral of ds / L_att(z, frequency_ghz) (GetTotalAttenuation*, .cc:134-219).
 * Departures: the integral is a fixed 24-node Gauss-Legendre rule in
 * s = sqrt(z - zv), zv = ln(B/(L-A))/C, where the reference calls QAGS at epsrel 1e-7; a refracted
 * leg ends at the turning depth of its own L, not at the reported zmax; a leg on which the
 * reference's integrand is NaN somewhere gives NaN.
 * Value c of pair i lands at d_out[c*ld + i], slot 0 then slot 1 in each pair of columns:
 *   0-1 time (s), 2-3 geometric path (m), 4-5 launch angle (deg), 6-7 receive angle (deg; -1000:
 *   no ray), 8-9 IgnoreCh (1: use the slot, 0: ignore it), 10-11 IncidenceAngleInIce (100, or the
 *   reflected ray's; not swapped), 12-13 AttRay, 14-15 RayType (1 D, 2 R, 3 Ra0, 4 Ra1; computed
 *   and dropped by the reference), 16-17 focusing factor (0.0 where its condition is not met or
 *   d_rays_lower is NULL).
 * Status (also d_status, nullable): AIRICE_ICESOL_SLOT0 / _SLOT1 = IgnoreCh of the slot,
 * _STRAIGHT the straight-line rule fired, _FOCUS0 / _FOCUS1 the focusing factor's condition was met and its
 * formula set it (the closing rule, zR == zT and factor 0 == 0 -> 1, sets no bit), _NONFINITE alone for a row the solver flagged
 * AIRICE_ICERAY_NONFINITE, whose value columns are NaN and whose IgnoreCh and types are 0.
 * model3 as airice_iceray_launch; it must have B < 0 < C.  Pairs are independent.
 * Stream-ordered, no device allocation, exactly one kernel launch; n == 0 is AIRICE_OK and nothing
 * is launched.  AIRICE_EINVAL before any device call, with airice_last_error() naming the
 * argument: a null required pointer; ld, ld_rays or (with d_rays_lower) ld_lower < n; a non-finite
 * a0; a frequency_ghz that is not finite and positive; a model outside B < 0 < C. */
#define AIRICE_ICESOL_FIELDS 18
#define AIRICE_ICESOL_TIME 0
#define AIRICE_ICESOL_PATH 2
#define AIRICE_ICESOL_LAUNCH_ANGLE 4
#define AIRICE_ICESOL_RECEIVE_ANGLE 6
#define AIRICE_ICESOL_IGNORE 8
#define AIRICE_ICESOL_INCIDENCE 10
#define AIRICE_ICESOL_ATTENUATION 12
#define AIRICE_ICESOL_RAY_TYPE 14
#define AIRICE_ICESOL_FOCUSING 16
#define AIRICE_ICESOL_SLOT0 1
#define AIRICE_ICESOL_SLOT1 2
#define AIRICE_ICESOL_STRAIGHT 4
#define AIRICE_ICESOL_FOCUS0 8
#define AIRICE_ICESOL_FOCUS1 16
#define AIRICE_ICESOL_NONFINITE 128
int airice_icesol_launch(const double *model3, const double *d_z0, const double *d_x1,
                         const double *d_z1, const double *d_rays, size_t ld_rays,
                         const double *d_rays_lower, size_t ld_lower, size_t n, double a0,
                         double frequency_ghz, double *d_out, size_t ld, uint8_t *d_status,
                         void *stream);
/* The whole of it with every array on the host; focusing != 0 also solves the receivers 1 cm
 * lower.  n > 1: copies, iceray_kernel once per receiver set (once or twice), icesol_kernel once,
 * synchronises.  n == 1 runs where airice_scalar_mode says (the calling thread, or the same
 * kernels through the one-query slot). */
int airice_icesol_host(const double *model3, const double *z0, const double *x1, const double *z1,
                       size_t n, double a0, double frequency_ghz, int focusing, double *out,
                       size_t ld, uint8_t *status);

/* --- the two rays' ice attenuation over a frequency grid (no reference counterpart: a consumer of
 * GetRayTracingSolutions calls it once per bin of a pulse's spectrum) -------------------------------
 * For n pairs x n_freq frequencies in ONE launch of icesol_spectrum_kernel, over d_rays (the rows
 * airice_iceray_launch wrote, stride ld_rays) and d_sol (what airice_icesol_launch wrote for the
 * same pairs, stride ld_sol; only its two AIRICE_ICESOL_RAY_TYPE columns are read: the slots hold
 * the rays it chose, at whatever frequency it ran).  d_freq_ghz: n_freq doubles in device memory.
 * AttRay of pair i, slot s, bin k lands at d_att[(2*i + s)*ld_f + k]: a pair's spectrum is
 * contiguous in frequency; the padding [n_freq, ld_f) of a row is left alone.  It is
 * 1 - |a0 * integral of ds / L_att(z, d_freq_ghz[k])| where the slot holds a ray and 0.0 where it
 * does not, with airice_icesol_launch's 24-node rule: a node's depth, index, temperature and
 * weight are formed once per pair, and a bin costs one exp per node.  Against
 * airice_icesol_launch at the same frequency: within 1e-12 * max(1, |1 - AttRay|), not bit for
 * bit.  A frequency that is not finite and positive makes its bin NaN where the slot holds a ray
 * (it is not refused: the frequencies stay on the device); a pair whose solver row is
 * AIRICE_ICERAY_NONFINITE is NaN in every bin of both slots.
 * Stream-ordered, no device allocation, no synchronisation, exactly one kernel launch; n == 0 is
 * AIRICE_OK and nothing is launched.  AIRICE_EINVAL before any device call: a null pointer;
 * n_freq == 0 (or above 2^27); ld_f < n_freq; ld_rays < n or ld_sol < n; a non-finite a0; a model
 * outside B < 0 < C. */
int airice_icesol_spectrum_launch(const double *model3, const double *d_z0, const double *d_z1,
                                  const double *d_rays, size_t ld_rays, const double *d_sol,
                                  size_t ld_sol, size_t n, double a0, const double *d_freq_ghz,
                                  size_t n_freq, double *d_att, size_t ld_f, void *stream);
/* The whole of it with every array on the host: sol_out (AIRICE_ICESOL_FIELDS columns of stride
 * ld, without focusing) and status as airice_icesol_host at freq_ghz[0] -- so its two attenuation
 * columns are bin 0's --, att_out[(2*i + s)*ld_f + k] as above.  n > 1: copies, iceray_kernel
 * once, icesol_kernel once, icesol_spectrum_kernel once, one synchronisation.  n == 1 runs where
 * airice_scalar_mode says: on the calling thread from the same source with no launch (the
 * default), or through the same three kernels. */
int airice_icesol_spectrum_host(const double *model3, const double *z0, const double *x1,
                                const double *z1, size_t n, double a0, const double *freq_ghz,
                                size_t n_freq, double *sol_out, size_t ld, uint8_t *status,
                                double *att_out, size_t ld_f);

/* --- in-ice interpolation tables ---------------------------------------------------------------
 * IceRayTracing::MakeTable (IceRayTracing.cc:2614-2724) and GetInterpolatedValue (.cc:2727-2905):
 * per antenna a grid of transmitter positions (xT, zT), 13 numbers per position, and the bilinear
 * / inverse-distance read of it.  DESIGN.md §10 has the rules as tables.
 * The image of n_ant antennas' tables is ONE contiguous array of doubles, the same bytes on host
 * and device, whose base is AIRICE_ICETAB_ALIGN-byte aligned:
 *   header  n_ant descriptors of AIRICE_ICETAB_DESC doubles {x_start, z_start, x_step, z_step, nx,
 *           nz, first_record, rx_depth} (counts as exact doubles), zero-padded to a multiple of
 *           AIRICE_ICETAB_RECORD doubles;
 *   records AIRICE_ICETAB_RECORD doubles (128 B, one cache line) per grid position; record r is
 *           at image + 16 r, antenna a's position (ix, iz) is record first_record[a] + ix*nz + iz
 *           (the reference's ix*TotalStepsZ_O + iz), antenna 0's first record follows the header
 *           and each antenna's records follow the one before.  Slots 0..12
 *           (AIRICE_ICETAB_PARAMS) are GridZValueb[AntNum][0..12]: 0-5 time, path, launch angle,
 *           receive angle, attenuation, focusing of slot 0; 6-11 the same of slot 1; 12 the
 *           incidence angle in ice; -1000 where MakeTable stores -1000.  Slot 13 is the position's
 *           AIRICE_ICESOL_* status byte as a double, slots 14 and 15 are 0.0.
 * A grid position is x_start + x_step*ix, z_start + z_step*iz: a product, then a sum, each rounded,
 * everywhere (the bits of GridPositionXb / GridPositionZb).
 * Every argument check below returns AIRICE_EINVAL before any device call, and
 * airice_last_error() names the argument. */
#define AIRICE_ICETAB_DESC 8
#define AIRICE_ICETAB_RECORD 16
#define AIRICE_ICETAB_PARAMS 13
#define AIRICE_ICETAB_ALIGN 128
#define AIRICE_ICETAB_MAX_BUILD 32 /* antennas of one build (their descriptors are a kernel argument) */
#define AIRICE_ICETAB_CELL 1        /* lookup status: a cell was used */
#define AIRICE_ICETAB_IDW 2         /* at least one parameter took the inverse-distance branch */
#define AIRICE_ICETAB_BAD_ANTENNA 4 /* the antenna index is outside [0, n_ant) */
/* Host: MakeTable's grid (.cc:2617-2636) with the reference's widths (40 m, 20 m) and steps
 * (0.1 m): nx = 401, nz = 201; x_start = hit - 20, or 0 when hit <= 20; z_start = depth - 10, or
 * -20 when |depth| <= 10 or depth + 10 >= 0.  first_record is left 0 (airice_icetab_layout). */
int airice_icetab_grid_init(double shower_hit_distance, double shower_depth, double rx_depth,
                            double *desc8);
/* Host: any grid; nx < 2, nz < 2 or a step that is not finite and positive is AIRICE_EINVAL. */
int airice_icetab_grid(double x_start, double z_start, double x_step, double z_step, int32_t nx,
                       int32_t nz, double rx_depth, double *desc8);
/* Host: fills first_record of the n_ant descriptors; *n_doubles = the image's size. */
int airice_icetab_layout(double *descs, size_t n_ant, size_t *n_doubles);
/* Host: the pack rule (.cc:2664-2715) for n positions: columns sol18[c*ld + i] (the 18
 * AIRICE_ICESOL_* columns, with focusing) and status[i] in, records[16 i .. 16 i + 15] out.
 * Focusing factor k is column 16+k when AIRICE_ICESOL_FOCUSk is set and the value is not NaN, else
 * 1.0; a slot whose IgnoreCh is 0 packs as -1000, slot 12 is -1000 when IncidenceAngleInIce[1]
 * is 100. */
int airice_icetab_pack_host(const double *sol18, size_t ld, const uint8_t *status, size_t n,
                            double *records);
/* Bytes of the work buffer of a build of these descriptors (after airice_icetab_layout). */
int airice_icetab_work_bytes(const double *descs, size_t n_ant, size_t *bytes);
/* The build: for all P = sum of nx*nz positions of n_ant <= AIRICE_ICETAB_MAX_BUILD antennas,
 * exactly four launches -- icetab_points_kernel (the header, and each position's (zT, xT, zR) and
 * (zT, xT, zR - 0.01) as 2P rows), iceray_kernel over the 2P rows (airice_iceray_launch),
 * icesol_kernel over P (airice_icesol_launch with the second P rows as d_rays_lower),
 * icetab_pack_kernel (one record per position, the rule of airice_icetab_pack_host).  descs is on
 * the HOST, as airice_icetab_layout left it; d_image and d_work are device memory.  Stream-ordered,
 * no device allocation.  AIRICE_EINVAL: a null pointer, n_ant == 0 or above the limit, a
 * misaligned image, work_bytes too small, and what airice_icesol_launch rejects (a non-finite a0,
 * a frequency_ghz that is not finite and positive, a model outside B < 0 < C). */
int airice_icetab_build_launch(const double *model3, double *d_image, const double *descs,
                               size_t n_ant, double a0, double frequency_ghz, void *d_work,
                               size_t work_bytes, void *stream);
/* The same with the image on the host: allocates, builds, copies back, synchronises. */
int airice_icetab_build_host(const double *model3, double *h_image, const double *descs,
                             size_t n_ant, double a0, double frequency_ghz);
/* The lookup: ONE launch of icetab_lookup_kernel, one query per lane; query i reads antenna
 * d_ant[i] (int32; d_ant NULL: antenna 0) at (d_x[i], d_z[i]) and all 13 parameters land at
 * d_out[c*ld + i], c < 13 -- what 13 calls of GetInterpolatedValue return (.cc:2736-2816 statement
 * by statement).  A query outside the grid or on an upper stop, a NaN query and an antenna index
 * outside [0, n_ant) give -1000 thirteen times.  d_status (nullable): the AIRICE_ICETAB_* bits.
 * Stream-ordered, no device allocation; n == 0 is AIRICE_OK and launches nothing. */
int airice_icetab_lookup_launch(const double *d_image, size_t n_ant, const int32_t *d_ant,
                                const double *d_x, const double *d_z, size_t n, double *d_out,
                                size_t ld, uint8_t *d_status, void *stream);
/* The same function on the calling thread for any n, image and arrays in host memory; launches
 * nothing (the engine of the drop-in's GetInterpolatedValue). */
int airice_icetab_lookup_host(const double *h_image, size_t n_ant, const int32_t *ant,
                              const double *x, const double *z, size_t n, double *out, size_t ld,
                              uint8_t *status);

/* --- in-ice ray paths (IceRayTracing::GetFullDirectRayPath / GetFullReflectedRayPath /
 * GetFullRefractedRayPath, IceRayTracing.cc:1257-1712) -------------------------------------------
 * The x(z) polyline of every accepted ray of n pairs, over the rows airice_iceray_launch wrote, in
 * two launches: icepath_consts_kernel (one lane per (pair, kind) segment) and icepath_kernel (one
 * lane per sample).  One ray is (kind, z0, x1, z1, L, zmax), kind one of AIRICE_ICERAY_D / _R /
 * _RA0 / _RA1, zmax read by the refracted kinds only.  With the reference's flip applied (z0 > z1
 * swaps them and emits x1 - xn), h = 0.5 m and F(z) = fDnfR(z; A, B, +C, L), in its order:
 *   D   zn = z1 - 0.5 k while zn >= z0, xn = F(zn) - F(z0); then the closing sample at z0 (z0
 *       appears twice when z1 - z0 is a multiple of 0.5);
 *   R   zn = z1 + 0.5 k while zn <= 0, xn = 2 F(-1e-7) - F(zn) - F(z0); zn = -1e-7 - 0.5 k while
 *       zn >= z0, xn = F(zn) - F(z0); then the closing sample;
 *   Ra  as R with -zmax for the surface: leg 1 while zn <= -zmax, leg 2 from -zmax.
 * Departures: a downward leg's depth is start - 0.5 k rounded once (the reference
 * chains zn = zn - h: the same counts, depths within 1 ulp); no sample is dropped (n^2 - L^2 is
 * clamped at 0 where the reference skips a NaN), so a count depends on (z0, z1, zmax) alone; on a
 * refracted ray n(z) - L = (L - A) expm1(-C (|z| - zt)), zt the turning depth of L, without
 * cancellation.  A ray whose status bit is clear, an AIRICE_ICERAY_NONFINITE row and a pair with a
 * depth above 0 or below -50,000 m (the reference's 100,000 steps) have count 0.
 *
 * Segment s = 4 i + r (r = 0 D, 1 R, 2 Ra0, 3 Ra1 of pair i) owns slots [offsets[s], offsets[s+1])
 * of x and z and fills the first count[s] of them; the rest are left untouched.
 *
 * Plan (host only, no GPU needed): offsets[0 .. 4n], offsets[0] = 0.  Capacities: the exact count
 * for D and R (they depend on the depths alone); for Ra the reflected count + 1, which bounds it
 * for every zmax >= 0, so the launch needs no copy back of zmax and stays stream-ordered behind
 * the solver; 0 for a kind outside ray_mask (AIRICE_ICERAY_* bits), for a kind whose bit is clear
 * in status[i] (status nullable: every kind) and for the pairs above.  *work_bytes (nullable): the
 * size of the launch's workspace. */
int airice_icepath_plan(const double *z0 /* host */, const double *z1 /* host */,
                        const uint8_t *status /* host, nullable */, size_t n, int ray_mask,
                        int64_t *offsets /* host, 4n+1 */, size_t *work_bytes);
/* Stream-ordered, no device allocation, exactly the two kernels after the upload of the plan into
 * d_work (work_bytes device bytes, 16-byte aligned).  d_z0 / d_x1 / d_z1: n device doubles;
 * d_rays: the solver's 32 columns of stride ld_rays (columns 19-24 and 29 are read; a segment
 * whose bit is clear there, or whose count exceeds its capacity, has count 0); z0 / z1 / status /
 * offsets: host, as given to / filled by the plan (checked against it); d_count: 4n device int64;
 * d_x / d_z: cap >= offsets[4n] doubles each.  n == 0 or a plan of no samples is AIRICE_OK and
 * launches nothing (d_count is then not written); a null required pointer, ld_rays < n, a cap or
 * work_bytes that is too small, or offsets that are not the plan's is AIRICE_EINVAL before any
 * device call, and airice_last_error() names the argument. */
int airice_icepath_launch(const double *model3, const double *d_z0, const double *d_x1,
                          const double *d_z1, const double *d_rays, size_t ld_rays,
                          const double *z0, const double *z1, const uint8_t *status, size_t n,
                          int ray_mask, const int64_t *offsets, void *d_work, size_t work_bytes,
                          int64_t *d_count, double *d_x, double *d_z, size_t cap, void *stream);
/* The same with every array on the host (rays: the 32 columns airice_iceray_host returned): copies,
 * launches and synchronises. */
int airice_icepath_host(const double *model3, const double *z0, const double *x1, const double *z1,
                        const double *rays, size_t ld_rays, const uint8_t *status, size_t n,
                        int ray_mask, const int64_t *offsets, int64_t *count, double *x, double *z,
                        size_t cap);
/* One ray on the calling thread, from the source the kernels are compiled from; no GPU (the
 * engine of the drop-in's GetFull*RayPath).  kind: one AIRICE_ICERAY_* ray bit.  *count = the
 * ray's samples; x / z (cap doubles each) receive them; a cap below the count is AIRICE_EINVAL. */
int airice_icepath_one_host(const double *model3, int kind, double z0, double x1, double z1,
                            double L, double zmax, double *x, double *z, size_t cap,
                            int64_t *count);

/* Device bookkeeping (thin wrappers so ctypes callers need no HIP runtime binding). */
int airice_device_count(int *count);
int airice_set_device(int device);
int airice_malloc(void **ptr, size_t bytes);
int airice_free(void *ptr);
int airice_memcpy_h2d(void *dst, const void *src, size_t bytes);
int airice_memcpy_d2h(void *dst, const void *src, size_t bytes);
int airice_synchronize(void);

/* Host assembly of tables (MakeRayTracingTable keeps AllTableAllAntData in host memory,
 * .cc:2101-2136): copy n_rays entries of the 11 float columns of a device table (column stride
 * d_ld) into a host table (column stride h_ld), stream-ordered (one 2-D DMA: hipMemcpy2DAsync).
 * h_table should be pinned (hipHostMalloc'd or registered with airice_host_register) for the copy
 * to be asynchronous at full PCIe rate.  A rank of a sharded build copies its row slab to
 * h_table + (first ray of the slab). */
int airice_table_to_host(const float *d_table, size_t d_ld, size_t n_rays, float *h_table,
                         size_t h_ld, void *stream);
/* Page-lock an existing host range for DMA (hipHostRegister, portable) / undo it. */
int airice_host_register(void *ptr, size_t bytes);
int airice_host_unregister(void *ptr);

/* --- table persistence (no reference counterpart: the reference keeps
 * AllTableAllAntData in memory only, .cc:2101-2136) -------------------------------------------
 * One antenna's host table in a file: a 512-byte little-endian header (magic "AIRTBL01", the
 * medium and grid it was traced with, the entry count, a 64-bit checksum of the column bytes),
 * then the 11 float32 columns of n_rays entries each, column after column.  Host-only (no GPU
 * needed); a device table goes through airice_table_to_host first. */
#define AIRICE_TABLE_FILE_HEADER 512
typedef struct airice_table_file_info {
  airice_medium medium; /* the medium the table was traced in */
  airice_grid grid;     /* its grid; n_rays = table_rows x angle_steps for a whole table */
  uint64_t n_rays;      /* entries per column */
  uint64_t checksum;    /* of the 11 columns' bytes (airice_table_checksum) */
} airice_table_file_info;
/* 64-bit checksum of n_rays entries of the 11 columns (column stride ld). */
uint64_t airice_table_checksum(const float *h_table, size_t ld, size_t n_rays);
int airice_table_save(const char *path, const airice_medium *m, const airice_grid *g,
                      const float *h_table, size_t ld, size_t n_rays);
/* Header of a table file (validated: magic, version, sizes against the file length). */
int airice_table_file_read_info(const char *path, airice_table_file_info *info);
/* Load a table file into h_table (column stride ld >= the file's n_rays), verifying its checksum.
 * expect (nullable): the medium the caller traces with -- a file traced in another medium (any
 * parsed field differs) is rejected with AIRICE_EINVAL.  info (nullable) receives the header. */
int airice_table_load(const char *path, const airice_medium *expect, float *h_table, size_t ld,
                      airice_table_file_info *info);

/* Kernel timing (bench.py's roofline legs; no reference counterpart).  When on, each launch
 * of a timed kernel is bracketed by a hipEvent pair on its own stream.  Names:
 * "table_kernel", "roots_kernel" (roots_kernel / roots_sorted_kernel, the minimizer's root
 * finder), "group_passes" (the batch-wide grouping passes), "out_kernel" (solve_out /
 * hdtip_out / trace_out), "lookup_kernel", "lookup_multi_kernel"
 * (airice_table_lookup_launch_multi), "ray_consts_kernel" and "ray_paths_kernel" (the two
 * kernels of airice_ray_paths_launch), "air2ice_kernel" (airice_air2ice_launch), "iceray_kernel"
 * (airice_iceray_launch), "icesol_kernel" (airice_icesol_launch), "icetab_points_kernel",
 * "icetab_pack_kernel" (airice_icetab_build_launch), "icetab_lookup_kernel"
 * (airice_icetab_lookup_launch), "icepath_consts_kernel" and "icepath_kernel" (the two kernels of
 * airice_icepath_launch), "icesol_spectrum_kernel" (airice_icesol_spectrum_launch),
 * "iceair_kernel" (airice_iceair_launch), "icefirst_geom_kernel" and "icefirst_select_kernel"
 * (the two kernels airice_icefirst_launch puts around "iceray_kernel").
 * airice_kernel_time waits for the recorded pairs
 * and returns their summed duration and count; reset != 0 clears them. */
int airice_kernel_timing(int on);
int airice_kernel_time(const char *name, double *total_ms, int64_t *launches, int reset);

/* Launch counters (no reference counterpart; always on, one atomic increment per launch): how
 * many times a kernel was launched in this process since the last reset, so a test can prove the
 * device path it checks really ran.  Names: "table_kernel", "rays_kernel", "scalar_ray_kernel",
 * "roots_kernel" (roots_kernel / roots_sorted_kernel), "scalar_solve_kernel" (the one-query
 * minimizer entry points in AIRICE_SCALAR_DEVICE mode), "out_kernel", "lookup_kernel",
 * "rtf_kernel" (ray layer and the GSL-Brent search), "single_ray_kernel", "path_kernel",
 * "ray_consts_kernel", "ray_paths_kernel" (airice_ray_paths_launch), "lookup_multi_kernel"
 * (airice_table_lookup_launch_multi; it does not count as "lookup_kernel"), "air2ice_kernel"
 * (airice_air2ice_launch; it does not count as "rtf_kernel"), "air_part_kernel" (the fill of a
 * table launch's air record, below; it does not count as "table_kernel"), "iceray_kernel"
 * (airice_iceray_launch), "icesol_kernel" (airice_icesol_launch), "icetab_points_kernel",
 * "icetab_pack_kernel" (airice_icetab_build_launch), "icetab_lookup_kernel"
 * (airice_icetab_lookup_launch), "icepath_consts_kernel", "icepath_kernel"
 * (airice_icepath_launch), "icesol_spectrum_kernel" (airice_icesol_spectrum_launch),
 * "iceair_kernel" (airice_iceair_launch), "icefirst_geom_kernel" and "icefirst_select_kernel"
 * (airice_icefirst_launch, whose solve counts as "iceray_kernel").
 * AIRICE_LAUNCH_REPORT=1 in the environment prints every count to stderr when the library
 * unloads. */
int airice_launch_count(const char *name, int64_t *count, int reset);

/* The table launch's per-grid caches on the current device (no reference counterpart; tests and
 * diagnostics).  out[0..2]: row-constant keys seen, of them filled (device buffer resident),
 * pinned (used by a launch captured into a graph); out[3..5]: the same for the start-angle
 * sines.  A grid's first launch only records its key; the second fills the buffers, stream-ordered
 * (INTEGRATION.md §5). */
int airice_table_cache_stats(int out[6]);

/* The table launch's air record (no reference counterpart).  The path of a table ray through the
 * air depends on the medium, the ice height, the Tx height and the launch angle, not on the
 * antenna: airice_table_launch keeps it per ray (32 bytes) for a launch -- medium, ice height,
 * grid and row range -- it has seen before, and later 11-column builds of that launch, for any
 * antenna depth, trace the ice segment only.  First use of a launch records its key, the second
 * fills the record (air_part_kernel, stream-ordered), later ones read it; tables are bit for bit
 * the uncached ones.  Launches with the 18-double output and airice_table_launch_multi do not use
 * it.
 * airice_air_cache_stats: out[0..3] = keys seen, records filled, records pinned by a captured
 * launch, bytes of device memory held, on the current device; out[4..5] = the limits below.
 * airice_air_cache_limits: a record above entry_bytes is never cached, the records of one device
 * hold at most total_bytes (least recently used unpinned records are freed first); a negative
 * value keeps a limit, total_bytes = 0 turns the cache off and drops every unpinned record
 * and key.  A record of 2^32 bytes or more (2^27 rays) is never cached, whatever entry_bytes
 * says: the kernels address a record with 32-bit offsets.  Defaults: 320 MiB and 640 MiB;
 * AIRICE_AIR_CACHE_MB=<n> in the environment sets the total (0: off). */
int airice_air_cache_stats(int64_t out[6]);
int airice_air_cache_limits(int64_t entry_bytes, int64_t total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* AIRICE_H */
