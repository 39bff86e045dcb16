/*
 * msweep_core.h -- C ABI of the MI355X-native abundance-estimation core (libmsweep_core.so).
 *
 * This is the drop-in boundary for mSWEEP's estimation hot path.  Every entry point cites
 * the reference interface (file:line under /root/reference) it replaces.  Plain pointers
 * and sizes only; all pointers are HOST pointers unless a name ends in `_dev`.  Return
 * value 0 = success, non-zero = error (text via msw_last_error); the C++ shim
 * (msweep_amd/cpp/rcgpar_hip.hpp) turns non-zero into std::runtime_error so that
 * mSWEEP's try/catch blocks (src/mSWEEP.cpp:400-406, 506-511) behave as with rcgpar.
 *
 * Threading: distinct handles may be used concurrently from distinct threads; one handle is used by one thread at
 * a time (the reference calls from its single main thread, src/mSWEEP.cpp:402,507).  A handle is bound to one HIP
 * device, and so are the alignments and read files made through it: every entry that takes one of them makes that
 * device current for the calling thread before it touches HIP, so threads whose handles sit on different devices do
 * not disturb each other, and a caller that uses HIP itself finds the device of the last handle it passed as the
 * current one.  An object made through a handle (msw_alignment_read_device, msw_fastq_open) is used by the thread that
 * uses the handle.  Error texts are per handle (msw_last_error(h)) or per thread (msw_last_error(NULL),
 * msw_alignment_last_error, msw_comm_last_error).  Nothing else in the library is shared between handles except the
 * code objects and the table of dynamic-LDS limits asked for (a limit belongs to a kernel on a device; the table only
 * raises it, under a lock: msweep_amd/csrc/lds_grants.hpp).  The developer switches (MSWEEP_* in the environment) are
 * read with getenv at the call: set them before the first thread starts.
 */
#ifndef MSWEEP_CORE_H
#define MSWEEP_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msw_core *msw_handle;

/* --algorithm (src/mSWEEP.cpp:127,192-204): rcggpu -> MSW_ALGO_RCG, emgpu -> MSW_ALGO_EM. */
enum { MSW_ALGO_RCG = 0, MSW_ALGO_EM = 1 };
/* --emprecision (src/mSWEEP.cpp:129,202; MSW_ALGO_EM only -- RCG ignores it, as rcgpar's rcg_optl_* have no such
 * argument).  MSW_PREC_FLOAT (round 5) is REAL fp32 arithmetic (msweep_amd/csrc/em_f32_kernels.hpp): likelihood values,
 * weights, row sums and quotients in fp32, the log-likelihood rounded to float once per iteration for the stop rule
 * (which is why a float run stops after a few hundred iterations where double reaches --max-iters, as the reference's
 * does: docs/gpubenchmarks.md:20-22), column sums in exact 64-bit fixed point.  Served by fp32 kernels on one GPU, for
 * likelihoods in CSR-of-ECs form with at most 6144 groups whose group vectors the sweeps keep in LDS, laid out as
 * 4-byte offset records with the whole slot table in LDS, or as index records (the layout of groupings with sizes up
 * to hundreds, whose fp64 slot table does not fit LDS) whenever the float image -- 4 bytes per slot-area entry, 12 per
 * group -- fits the 160 KB of LDS.  Other layouts (8-byte / value records, index records beyond that, dense matrices
 * without background structure, EC-sharded solves) run the fp64 kernels under MSW_PREC_FLOAT as until round 4 --
 * msw_timing::em_float_kernels says which it was. */
enum { MSW_PREC_DOUBLE = 0, MSW_PREC_FLOAT = 1 };

/* ---- lifetime ---------------------------------------------------------------------- */
int msw_core_create(int device, msw_handle *out);
void msw_core_destroy(msw_handle h);
/* last error text of the handle (or of the failed msw_core_create when h == NULL) */
const char *msw_last_error(msw_handle h);
/* library / device identification string ("msweep_core <ver> gfx950 ...") */
const char *msw_core_version(void);

/* ---- likelihood upload -------------------------------------------------------------
 * Replaces the materialised `seamat::DenseMatrix<double> log_likelihoods`
 * (include/Likelihood.hpp:85,176-185) that rcg_optl receives as `ll_mat`
 * (src/mSWEEP.cpp:176,402,507).  The likelihood stays resident on the device across the
 * 1 + --iters solves of one grouping (same `logl` object at :402 and :507).            */

/* Dense G x E, rows = groups, element (g, j) at L[g*ld + j] -- the seamat layout read via
 * operator()(row, col) (include/Likelihood.hpp:182,265); needed for --read-likelihood
 * (include/Likelihood.hpp:224-253).
 * A matrix of the shape fill_ll_mat writes (include/Likelihood.hpp:176-185: one background value,
 * log(zi), in at least 3/4 of the cells and at most 65536 distinct values elsewhere) is re-expressed
 * on the device as the CSR-of-ECs form below -- the same numbers, bit for bit
 * (msw_core_get_dense_logl returns the input), any group count, solved by the sparse sweeps.
 * Any other matrix is kept dense up to n_groups = 8192; beyond, it is re-expressed whatever its shape (every
 * cell that differs from the most frequent value listed, up to 2^28 of them).  msw_core_shape's nnz tells which. */
int msw_core_set_dense_logl(msw_handle h, const double *L, size_t n_groups, size_t n_ecs,
                            size_t ld);

/* CSR-of-ECs form of the same matrix: for EC j the cells k in [rowptr[j], rowptr[j+1])
 * name group grp[k] hit cnt[k] >= 1 times; L(g, j) = lut[g*lut_ld + cnt] and every cell
 * not listed is `logzi` (= lut[g*lut_ld + 0] for every g, include/Likelihood.hpp:98).
 * `lut` is the precalc_lls table (include/Likelihood.hpp:92-107). */
int msw_core_set_csr(msw_handle h, const uint64_t *rowptr, const uint32_t *grp,
                     const uint32_t *cnt, const double *lut, size_t lut_ld, double logzi,
                     size_t n_groups, size_t n_ecs);

/* Builds the CSR-of-ECs likelihood on the device straight from the pseudoalignment:
 * replaces LL_WOR21::fill_ll_mat + fill_ec_counts (include/Likelihood.hpp:109-195) and
 * ConstructAdaptiveLikelihood (:333-380).
 *   ec_tptr/ec_targets : for EC i the targets it aligned to (the set bits of
 *                        Alignment::operator()(i, j), include/mSWEEP_alignment.hpp:223)
 *   target_group[T]    : Alignment::get_groups() (include/mSWEEP_alignment.hpp:241)
 *   group_sizes[G]     : Grouping::get_sizes()   (include/Grouping.hpp:35-50)
 *   ec_counts[E]       : Alignment::reads_in_ec  (include/mSWEEP_alignment.hpp:220)
 *   q, e               : -q / -e flags (bb_constants, include/Likelihood.hpp:212-214)
 *   min_hits           : --min-hits mask (include/Likelihood.hpp:141-171)
 * Outputs: *n_groups_out = groups kept, mask_out[G] = groups_considered() (:331),
 * logc_out[E] = log_counts() (:328); either may be NULL.
 * EC-sharded (msw_core_set_comm called first; every rank passes its own block of ECs and the same targets /
 * groups): the --min-hits counts are all-reduced (G unsigned 64-bit integers, once), so every rank keeps
 * the same groups in the same order. */
int msw_core_build_likelihood(msw_handle h, const uint64_t *ec_tptr,
                              const uint32_t *ec_targets, size_t n_ecs,
                              const uint32_t *target_group, size_t n_targets,
                              const uint64_t *group_sizes, size_t n_groups,
                              const uint64_t *ec_counts, double q, double e,
                              double zero_inflation, size_t min_hits,
                              size_t *n_groups_out, uint8_t *mask_out, double *logc_out);

/* Downloads the dense G' x E log-likelihood (rows = groups) of the resident likelihood --
 * what Likelihood::log_mat() (include/Likelihood.hpp:325) would hold; used by
 * --write-likelihood (include/Likelihood.hpp:255-273) and the parity tests. */
int msw_core_get_dense_logl(msw_handle h, double *L_out, size_t ld);
/* FNV-1a hash of the resident CSR-of-ECs layout (EC order, slice geometry, records): test hook that
 * holds the device packer against its host reference implementation (MSWEEP_HOST_PACK=1). */
int msw_core_layout_hash(msw_handle h, uint64_t *hash_out);
/* shape of the resident likelihood */
int msw_core_shape(msw_handle h, size_t *n_groups, size_t *n_ecs, size_t *nnz);
/* How the resident CSR-of-ECs likelihood is laid out for the sweeps: reporting only (bench.py, the
 * timing tools); no reference counterpart. */
typedef struct msw_layout_info {
  int32_t record_bytes;        /* 4 or 8 bytes per listed cell; 12: value records (the cell's log-likelihood inline) */
  int32_t index_records;       /* 1: (group, entry) index records + hybrid slot area; 0: byte-offset records */
  int32_t groups_in_lds;       /* the per-group vectors of both sweeps live in LDS */
  int32_t table_in_lds;        /* the whole slot area lives in LDS */
  int32_t passB_mode;          /* k_passB GMODE (sweep_kernels.hpp) */
  uint32_t slot_entries;       /* 16-byte entries of the slot area */
  uint32_t slot_entries_in_lds;
  uint32_t n_slices, n_long_ecs;
  uint64_t rows;               /* slice rows (64 records each), padding included */
  uint64_t rows_from_memory;   /* ... whose table entries are gathered from memory (cold segments, whole slices) */
  uint32_t slices_by_lanes[7]; /* slices whose ECs take 64, 32, 16, 8, 4, 2, 1 lanes each (ECs of 513..1024, 257..512,
                                * .., 17..32, <= 16 cells; MSWEEP_MULTILANE=0: all in the last) */
  uint32_t max_rows;           /* rows of the longest slice (<= 16: every slice on the register path of the sweeps) */
  int32_t bank_scheduled;      /* the cells of every slice were ordered for the LDS banks (msw_core_set_pack_schedule) */
  int32_t passB_reg_cells;     /* records per slice lane pass B holds in registers: 16, or 8 = its short-slice instantiation
                                * with 16 wavefronts per workgroup (slices of > 8 rows hold <= 1/20 of the rows) */
  uint64_t rows_over_8;        /* rows of the slices of more than 8 rows (0 when not counted: index / wide / value records) */
  int32_t passB_waves;         /* wavefronts per workgroup of the k_passB instantiation this layout is swept with */
  int32_t pad_;
} msw_layout_info;
int msw_core_layout_info(msw_handle h, msw_layout_info *out);
/* Whether the NEXT likelihood made resident on the handle (msw_core_set_csr, msw_core_build_likelihood, a dense
 * matrix re-expressed as CSR-of-ECs) gets its cells ordered for the LDS banks of the sweeps (the order of
 * the cells inside an EC is free).  enabled = 1 (default): an iteration is 5-6 % faster (cfg3: 0.177 against 0.187 ms)
 * and the upload 10 ms slower (cfg3; 28 ms at cfg5) -- pays from about the 1 000th iteration on the same likelihood,
 * i.e. for bootstrap runs (src/mSWEEP.cpp:496-518); enabled = 0: the cells keep their CSR order -- the faster way to
 * ONE solve.  Same results either way (the order of the additions inside an EC changes: rounding).  The drivers set
 * it from --iters.  No reference counterpart. */
int msw_core_set_pack_schedule(msw_handle h, int enabled);

/* ---- solver options ------------------------------------------------------------------
 * The knobs of the optimiser loops that are restated from memory of rcgpar v1.2.1 (the library is an un-vendored
 * FetchContent dependency of the reference, CMakeLists.txt:274-311).  The defaults are the
 * restatement; every alternative reading is selectable, here and in the oracle (oracle/msweep_oracle.h
 * orc_rcg_opts / orc_em_opts), so that a result from a real mSWEEP run can decide between them
 * (tests/golden/external/README.md).  Options persist on the handle and apply to every later solve and bootstrap.
 *   MSW_OPT_CHECK_EVERY n  the stop rule `bound - oldbound < tol && !didreset` (and EM's) is tested after iterations
 *                          n, 2n, ... only.  Default 1.  (Every iteration count the reference publishes is a multiple
 *                          of 5, docs/gpubenchmarks.md:15-25: rcgpar logs every 5th iteration -- the default's
 *                          reading -- or tests on that grid, n = 5.)
 *   MSW_OPT_INIT_BOUND  b  the value `bound` holds before the first iteration; default -100000 (a first bound below
 *                          it sends iteration 0 through the steepest-descent retry).
 *   MSW_OPT_EM_PRIOR 0|1   em_torch's M-step: 0 = MAP, the Dirichlet prior as pseudo-counts alpha0 - 1 (default);
 *                          1 = ML, theta_g = sum_j c_j q_gj / sum_j c_j (alpha0 ignored).
 *   MSW_OPT_EM_STOP  0|1   em_torch's stop: 0 = gain of the count-weighted log-likelihood < tol (default);
 *                          1 = largest move of a mixture weight in the M-step < tol. */
enum { MSW_OPT_CHECK_EVERY = 0, MSW_OPT_INIT_BOUND = 1, MSW_OPT_EM_PRIOR = 2, MSW_OPT_EM_STOP = 3 };
int msw_core_set_option(msw_handle h, int option, double value);
int msw_core_get_option(msw_handle h, int option, double *value);

/* ---- solve --------------------------------------------------------------------------
 * Replaces rcgpar::rcg_optl_torch / rcg_optl_omp / em_torch as called from rcg_optl()
 * (src/mSWEEP.cpp:176-205) followed by rcgpar::mixture_components[_torch]
 * (src/mSWEEP.cpp:419-423, 512-516):
 *   logc[E]   = log_times_observed (natural log of EC counts; -inf allowed,
 *               src/BootstrapSample.cpp:70)
 *               NULL = the log counts msw_core_build_likelihood left on the device (no 8 * E
 *               byte upload per solve; an error for likelihoods that were uploaded instead)
 *   alpha0[G] = prior_counts (src/mSWEEP.cpp:391-398)
 *   tol, max_iters = --tol / --max-iters (src/mSWEEP.cpp:123-125)
 * theta_out[G] receives mixture_components(gamma, logc).  iters_out / bound_out optional. */
int msw_core_solve(msw_handle h, const double *logc, const double *alpha0, double tol,
                   size_t max_iters, int algo, int prec, double *theta_out,
                   size_t *iters_out, double *bound_out);

/* The same call split in two for callers that keep the inputs resident (bench.py's timed
 * region, the bootstrap driver): msw_core_prepare uploads logc / alpha0 and forms the EC
 * multiplicities on the device; msw_core_run executes the optimiser on the prepared inputs.
 * msw_core_solve == msw_core_prepare + msw_core_run. */
int msw_core_prepare(msw_handle h, const double *logc, const double *alpha0);
int msw_core_run(msw_handle h, double tol, size_t max_iters, int algo, int prec,
                 double *theta_out, size_t *iters_out, double *bound_out);

/* The G x E log-responsibility matrix gamma of the last solve (the DenseMatrix rcg_optl
 * returns, src/mSWEEP.cpp:195,199,203; consumed by Sample::store_probs / write_probs /
 * mGEMS binning, src/mSWEEP.cpp:402,451,478-487).  Row-major, rows = groups, leading
 * dimension ld >= E.  Materialised on demand from the structured state. */
int msw_core_gamma(msw_handle h, double *gamma_out, size_t ld);

/* The columns [ec_begin, ec_end) of the same matrix: gamma_out[g * ld + (j - ec_begin)], ld >= ec_end -
 * ec_begin.  What Sample::write_probs (src/Sample.cpp:63-85: one output line per EC) and the mGEMS binning
 * input (src/mSWEEP.cpp:437-469) consume EC by EC: at the size of BASELINE's configurations the whole matrix
 * is hundreds of GB (G x E x 8 B = 375 GB at 10 M reads x 5 k groups), a block of it is not. */
int msw_core_gamma_block(msw_handle h, size_t ec_begin, size_t ec_end, double *gamma_out, size_t ld);

/* mGEMS read binning (src/mSWEEP.cpp:437-469, mGEMS::BinFromMatrix) on the device, from the last solve: the reads of
 * EC j go to the bin of target k when gamma(targets[k], j) >= log(thresholds[k]) -- the gamma msw_core_gamma_block
 * returns, bit for bit, and log(t_k) formed on the host.  Within a bin: ECs in EC order, the reads of an EC as
 * ec_reads holds them (Alignment::get_aligned_reads, include/mSWEEP_alignment.hpp:224).
 *   ec_rptr[n_ecs + 1] / ec_reads[ec_rptr[n_ecs]]  the read ids of every EC (msw_alignment_export); n_ecs = the handle's E
 *   targets[n_targets]     rows of the kept groups (0 .. n_groups_out - 1), each at most once
 *   thresholds[n_targets]  probabilities t_k in [0, 1] (the drivers pass 1 - theta_k)
 *   bin_ptr[n_targets + 1] always written: bin k = reads_out[bin_ptr[k] .. bin_ptr[k + 1])
 *   reads_out              NULL: sizes only; else bin_ptr[n_targets] read ids
 *   log_thr_out            optional: the log(t_k) the comparison used
 * Device memory O(E + pairs + output), never G x E; an output that cannot be allocated is an error naming the bytes.
 * Refused (non-zero, msw_last_error): no solve yet, n_ecs != E, a target out of range or repeated, a threshold NaN or
 * outside [0, 1], the dense flavour (set_dense_logl with MSWEEP_DENSE_COMPRESS=0), a communicator set.  Every call runs
 * the whole pass (nothing is cached between a sizes call and a fill call). */
int msw_core_bin_reads(msw_handle h, const uint64_t *ec_rptr, const uint32_t *ec_reads, size_t n_ecs,
                       const uint32_t *targets, const double *thresholds, size_t n_targets, uint64_t *bin_ptr,
                       uint32_t *reads_out, double *log_thr_out);
/* The same on an alignment handle: classes resident on h's device (msw_alignment_read_device) are read where they lie,
 * any other handle's host arrays are uploaded. */
struct msw_alignment;
int msw_core_bin_reads_aln(msw_handle h, struct msw_alignment *a, const uint32_t *targets, const double *thresholds,
                           size_t n_targets, uint64_t *bin_ptr, uint32_t *reads_out, double *log_thr_out);

/* What `mGEMS bin` gives beyond the target bins (docs/pipeline.md:54-64), on the device, from the last solve
 * (msweep_amd/csrc/assign_kernels.hpp; DESIGN.md 7h, [UPSTREAM-UNVERIFIED] like the rule of msw_core_bin_reads): every EC
 * is judged against ALL estimated groups, pass(g, j) <=> gamma(g, j) >= log(thresholds[g]) with the gamma
 * msw_core_gamma_block returns and log formed on the host; a NaN compares false.
 *   thresholds[n_groups]   t_g in [0, 1] for EVERY estimated group (the drivers pass 1 - theta_g)
 *   targets[n_targets]     rows of the groups whose bins are wanted, each at most once; n_targets == 0 is valid
 *   flags                  MSW_ASSIGN_UNASSIGNED: bin_ptr has n_targets + 2 entries and bin n_targets holds the reads of
 *                          the ECs no group claims (n_assigned == 0), ECs in EC order -- reads that did not pseudoalign
 *                          are in no EC, hence not in it.  MSW_ASSIGN_KEEP_TABLE: the ECs' target lists and an index of
 *                          the reads by id stay on the handle for msw_core_assign_table_*
 *   bin_ptr / reads_out    as msw_core_bin_reads; the target bins ARE msw_core_bin_reads' for the same targets and
 *                          thresholds[targets[k]], id for id
 *   n_assigned_out[n_ecs]  optional: the groups, of all n_groups, that claim each EC
 *   class_reads_out[3]     optional: the reads in ECs claimed by 0, by 1 and by >= 2 groups
 * Device memory O(E + pairs + aligned reads + output); an allocation that fails is an error naming the bytes.  No atomic
 * decides an order: two calls give the same bytes.  Every call runs the whole pass.
 * Refused like msw_core_bin_reads (no solve yet, n_ecs != E, a target out of range or repeated, the dense flavour, a
 * communicator set), and for a threshold of ANY group that is NaN or outside [0, 1]. */
#define MSW_ASSIGN_UNASSIGNED 1u /* bin_ptr has n_targets + 2 entries; bin n_targets = the unassigned reads */
#define MSW_ASSIGN_KEEP_TABLE 2u /* keep the per-class target lists and the reads-by-id index on the handle */
int msw_core_assign_reads(msw_handle h, const uint64_t *ec_rptr, const uint32_t *ec_reads, size_t n_ecs,
                          const double *thresholds, const uint32_t *targets, size_t n_targets, unsigned flags,
                          uint64_t *bin_ptr, uint32_t *reads_out, uint32_t *n_assigned_out, uint64_t class_reads_out[3]);
/* The same on an alignment handle (as msw_core_bin_reads_aln). */
int msw_core_assign_reads_aln(msw_handle h, struct msw_alignment *a, const double *thresholds, const uint32_t *targets,
                              size_t n_targets, unsigned flags, uint64_t *bin_ptr, uint32_t *reads_out,
                              uint32_t *n_assigned_out, uint64_t class_reads_out[3]);
/* The read x target assignment table of the last msw_core_assign_reads[_aln] call with MSW_ASSIGN_KEEP_TABLE, as text
 * formatted on the device: one row per aligned read in ascending read id -- the (read id, EC) pairs in a stable sort by
 * id, so an id that host-supplied arrays list in two ECs gives two rows --, dec(id), then per target in target order
 * "\t1" if the read's EC passes it, else "\t0", then '\n'.  With n_targets == 0 the rows are bare ids.
 *   msw_core_assign_table_rows        the number of rows (the aligned reads)
 *   msw_core_assign_table_block       the rows [row_begin, row_end) in the handle's pinned text buffer (valid until the
 *                                     next text or table call)
 *   msw_core_assign_table_block_gzip  the same rows into the open gzip stream (msw_core_gzip_begin): the bytes to append
 *                                     to the file; text_len_out: their uncompressed length
 * The kept state is dropped by a new resident likelihood (set_*, build_*), a solve, a bootstrap, and an assign call
 * without MSW_ASSIGN_KEEP_TABLE.  Refused: no kept state, a row range out of bounds, a block whose worst-case text
 * (11 + 2 n_targets bytes per row) exceeds 1 GiB -- the message says how many rows fit --, the gzip variant without an
 * open stream. */
int msw_core_assign_table_rows(msw_handle h, size_t *n_rows_out);
int msw_core_assign_table_block(msw_handle h, size_t row_begin, size_t row_end, const char **text_out, size_t *len_out);
int msw_core_assign_table_block_gzip(msw_handle h, size_t row_begin, size_t row_end, const char **out, size_t *len_out,
                                     size_t *text_len_out);

/* --write-read-probs: the read-to-group probabilities of the last solve as SPARSE text formatted on the device
 * (sparse_probs_kernels.hpp): one line  dec(id) '\t' dec(g) '\t' g6(p) '\n'  per KEPT cell.  Cell (g, j) is kept iff
 * gamma(g, j) >= log(threshold) -- gamma the very bits msw_core_gamma_block returns, log(threshold) formed once on the
 * host (*log_thr_out), a NaN compares false --, g over the estimated groups (the rows of the resident likelihood), and
 * g6(p) is the token MSW_TEXT_PROBS prints for that cell, byte for byte (undecided cells completed on the host as there).
 * Since the probabilities of an EC sum to 1, an EC keeps at most 1 / threshold cells; they are found from its listed cells
 * and a prefix of the groups ordered by weight, never in G steps per EC.
 *   a == NULL  rows are ECs in the original EC order: id = ec_id, n_rows = E
 *   a != NULL  rows are the (read id, EC) pairs of a in the stable sort by read id, the rows of msw_core_assign_table_*:
 *              id = the read id, n_rows = the aligned reads.  Classes resident on h's device are read where they lie, any
 *              other handle's host arrays are uploaded.
 * Within a row the lines are in ascending g; a row without a kept cell gives no bytes; two calls give the same bytes.
 *   msw_core_sparse_probs_begin      selects (replaces an earlier selection); *n_rows_out: the rows
 *   msw_core_sparse_probs_next       the next whole rows whose text fits max_bytes (1 ... 1 GiB), in the handle's pinned text
 *                                    buffer (valid until the next text call); *rows_done_out: the rows handed out so far;
 *                                    *len_out == 0 with *rows_done_out == n_rows: finished.  *n_cells_out: the kept cells of
 *                                    the piece, *n_host_cells_out: those the host printed.  A single row larger than
 *                                    max_bytes is an error naming its size (a row is measured with its undecided cells 13
 *                                    bytes wide, as the device writes them); the selection stays where it was.
 *   msw_core_sparse_probs_next_gzip  the same inside the handle's open gzip stream (msw_core_gzip_begin ... _end), as
 *                                    msw_fastq_next_gzip: the bytes to append to the file; *text_len_out: the plain length
 *   msw_core_last_sparse_probs_timing  measurement hook (tools/sparse_probs_timing.py): device time of the kernels since
 *                                    begin (events on the handle's stream; copies and the gzip kernels are not in it), the
 *                                    bytes of text handed out and the kept cells
 * Device memory O(E + pairs + the candidates and text of a piece), never G x E; an allocation that fails is an error
 * naming the bytes.  The kept state is dropped by a new resident likelihood (set_*, build_*), a solve, a bootstrap and
 * msw_core_trim.  Refused (non-zero, msw_last_error, the handle stays usable): no solve yet, a threshold that is NaN,
 * <= 0 or > 1, an alignment whose EC count is not the handle's E, the dense flavour (MSWEEP_DENSE_COMPRESS=0), a
 * communicator set, next without begin, the gzip variant without an open stream. */
int msw_core_sparse_probs_begin(msw_handle h, struct msw_alignment *a, double threshold, uint64_t *n_rows_out,
                                double *log_thr_out);
int msw_core_sparse_probs_next(msw_handle h, size_t max_bytes, const char **text_out, size_t *len_out,
                               uint64_t *rows_done_out, uint64_t *n_cells_out, size_t *n_host_cells_out);
int msw_core_sparse_probs_next_gzip(msw_handle h, size_t max_bytes, const char **out, size_t *len_out,
                                    uint64_t *rows_done_out, size_t *text_len_out);
int msw_core_last_sparse_probs_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out, uint64_t *cells_out);

/* The text of the matrix outputs, formatted on the device (text_kernels.hpp): the lines of the ECs [ec_begin, ec_end)
 * as contiguous bytes in EC order, every cell printed as the reference's default `ostream <<` prints a double --
 * printf("%g"), byte for byte (g6_format.hpp).  Only the bytes cross the link; nothing is sized G x E.
 *   MSW_TEXT_PROBS   needs a solve; no line_prefix.  Line j: dec(j), then '\t' g6(exp(gamma(g, j))) per group, then
 *                    n_zero_cols times "\t0", then '\n' (Sample::write_probs, src/Sample.cpp:63-85,154-186).  exp is
 *                    the device's: against the host's exp a cell can differ where a rounding boundary of the six
 *                    digits lies between two neighbouring doubles.
 *   MSW_TEXT_LOGL    line_prefix[j - ec_begin] (the EC's read count) required, n_zero_cols == 0.  Line j: dec(prefix),
 *                    then '\t' g6(L(g, j)) per group, then '\n' (include/Likelihood.hpp:255-273); L = the bits
 *                    msw_core_get_dense_logl returns.
 *   MSW_TEXT_BITSEQ  no line_prefix, n_zero_cols == 0.  Per EC the part of the BitSeq line after the read id:
 *                    dec(G + 1) ' ', then dec(g + 1) ' ' g6(L(g, j)) ' ' per group, then "0 -10000.00\n"
 *                    (include/Likelihood.hpp:295-305).
 * *text_out points into a pinned host buffer owned by the handle, valid until the next call on the handle; *len_out is
 * its length.  n_host_cells_out (may be NULL): cells the host had to format (values the device routine leaves
 * undecided).  Refused (non-zero, msw_last_error; the handle stays usable): PROBS before a solve, a prefix missing or
 * superfluous, zero columns outside PROBS, a range out of bounds, and a range whose worst-case text
 * -- 20 + 14 G + 2 n_zero_cols + 12 bytes per line (BITSEQ: the group numbers on top) -- exceeds 1 GiB: the message
 * says how many classes fit. */
enum { MSW_TEXT_PROBS = 0, MSW_TEXT_LOGL = 1, MSW_TEXT_BITSEQ = 2 };
int msw_core_text_block(msw_handle h, int what, size_t ec_begin, size_t ec_end,
                        const uint64_t *line_prefix, size_t n_zero_cols,
                        const char **text_out, size_t *len_out, size_t *n_host_cells_out);
/* The formatter alone, its test and diagnostic entry: the n host doubles x through the same kernels, each followed by
 * '\n'.  text_out / len_out / n_host_out as above. */
int msw_core_format_g6(msw_handle h, const double *x, size_t n,
                       const char **text_out, size_t *len_out, size_t *n_host_out);
/* Measurement hook (tools/text_timing.py): device time of the text kernels of the last of those two calls -- length
 * pass, scan and write pass, from events on the handle's stream; the materialisation of the block and the copy of the
 * bytes are not in it -- and the bytes of text the kernels wrote (undecided cells still 13 blanks wide). */
int msw_core_last_text_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out);

/* --compress z / --compression-level (src/OutfileDesignator.cpp:30-37: the reference wraps its output files in a
 * compressing stream on the host): the text outputs as ONE ordinary single-member gzip file (RFC 1952 / RFC 1951)
 * whose DEFLATE stream is written on the device (deflate_kernels.hpp), where the text lies: only the compressed bytes
 * cross the link.  One stream may be open per handle.  Every call returns bytes to APPEND to the file: *out points into a
 * pinned host buffer owned by the handle, valid until the next call on the handle; *len_out may be 0.
 * The text of every call is cut into chunks of 32 KiB that are compressed on their own (no match crosses a chunk or a
 * call; each is one dynamic or stored block followed by an empty stored block, as pigz writes them), so the bytes are a
 * function of the text, the chunk size and the call boundaries alone.  Level 0 writes stored blocks; levels 1 ... 9 run
 * the SAME parse -- this core has one effort setting (greedy, single-entry hash buckets, dynamic codes).  The CRC-32 is
 * computed on the device at every level.
 * Calling append / text_block_gzip / end without an open stream, begin while one is open, or a level outside 0 ... 9 is
 * refused (non-zero, msw_last_error); the handle stays usable.
 * MSWEEP_HOST_GZIP=1 in the environment at begin (developer switch): the same calls bring the plain text to the host and
 * compress it with zlib at the requested level -- the reference's method, the other side of the A/B and of the tests. */
/* src/OutfileDesignator.cpp:30-37: opens the stream; returns the gzip header (mtime 0, OS 255). */
int msw_core_gzip_begin(msw_handle h, int level, const char **out, size_t *len_out);
/* src/OutfileDesignator.cpp:30-37 around the matrix writers: the arguments and the refusals of msw_core_text_block; returns
 * the compressed chunks of that text, its undecided cells put in on the device (a block with more of them than the
 * list holds: formatted by the host and uploaded).  *text_len_out (may be NULL): the uncompressed length. */
int msw_core_text_block_gzip(msw_handle h, int what, size_t ec_begin, size_t ec_end,
                             const uint64_t *line_prefix, size_t n_zero_cols,
                             const char **out, size_t *len_out, size_t *n_host_cells_out, size_t *text_len_out);
/* src/OutfileDesignator.cpp:30-37 around everything else the drivers write (header lines, the BitSeq lines per read, the
 * bins): n host bytes, uploaded and compressed through the same kernels.  n == 0 is valid; at most 1 GiB a call. */
int msw_core_gzip_append(msw_handle h, const char *bytes, size_t n, const char **out, size_t *len_out);
/* src/OutfileDesignator.cpp:30-37, the stream's destructor: the final block, CRC-32 and ISIZE; closes the stream. */
int msw_core_gzip_end(msw_handle h, const char **out, size_t *len_out);
/* Measurement hook (tools/gzip_timing.py): device time of the gzip kernels (parse, CRC, scan, emit; events on the handle's
 * stream) over the stream that is open or was closed last, the bytes of text it took and the bytes it returned. */
int msw_core_last_gzip_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_in_out, uint64_t *bytes_out_out);

/* Per-iteration diagnostics of the last solve (what rcgpar logs every 5th iteration to
 * the verbose stream, src/mSWEEP.cpp:198): arrays of length n (<= max recorded, 4096);
 * theta_trace is n x G or NULL.  Returns the number of iterations recorded via *n_out. */
int msw_core_trace(msw_handle h, size_t n, double *bound, double *newnorm, double *beta,
                   int32_t *didreset, double *theta_trace, size_t *n_out);
/* how many leading iterations keep a theta snapshot (default 0) */
int msw_core_set_trace_theta(msw_handle h, size_t n_iters);

/* ---- bootstrap ----------------------------------------------------------------------
 * Replaces BootstrapSample::init_bootstrap / construct / resample_counts
 * (src/BootstrapSample.cpp:33-73) and the replicate loop (src/mSWEEP.cpp:496-518).
 *   ec_counts[E]      Alignment::reads_in_ec as uint32 (src/BootstrapSample.cpp:38-42)
 *   seed              --seed narrowed to int32 (include/Sample.hpp:169,172)
 *   bootstrap_count   draws per replicate (src/BootstrapSample.cpp:56)
 *   replicates [rep_begin, rep_end) of the ONE sequential mt19937_64 stream are solved
 *   (a rank of an N-GPU job passes its own slice; the stream position of replicate b is
 *   b * bootstrap_count draws).
 * theta_out is (rep_end - rep_begin) x G, row b = abundances of replicate rep_begin+b,
 * normalised by the resampled total as src/mSWEEP.cpp:513 does.  iters_out optional.
 * A replicate whose solve fails numerically (likelihood underflow, non-finite bound: the cases in which
 * the reference writes NaN abundances) yields a row of NaN and the call still returns 0 -- the other
 * replicates are unaffected; device errors and bad arguments fail the whole call. */
int msw_core_bootstrap(msw_handle h, const uint32_t *ec_counts, int32_t seed,
                       size_t bootstrap_count, size_t rep_begin, size_t rep_end,
                       const double *alpha0, double tol, size_t max_iters, int algo,
                       int prec, double *theta_out, size_t *iters_out);

/* The whole replicate loop of src/mSWEEP.cpp:496-518 over the GPUs of one node: rank r of `comm`
 * (msw_comm_create_rccl: one process per GPU; msw_comm_create_local: thread-ranks) solves the contiguous
 * block [n_replicates * r / P, n_replicates * (r + 1) / P) of the one sequential stream and ONE all-gather
 * (RCCL over xGMI) leaves the complete n_replicates x G block in replicate order -- the rows
 * 1..n_replicates of bootstrap_results (include/Sample.hpp:157,180) -- on EVERY rank; results do not
 * depend on the number of ranks (more ranks than replicates: the surplus ranks solve nothing and still take
 * part in the exchange).  Every rank holds the same resident likelihood and passes the same
 * arguments.  iters_out[n_replicates] optional.  A rank whose block fails still joins the all-gather and
 * reports through a status word: the call then returns non-zero on EVERY rank and no rank is left waiting. */
struct msw_comm;
int msw_core_bootstrap_dist(msw_handle h, struct msw_comm *comm, const uint32_t *ec_counts, int32_t seed,
                            size_t bootstrap_count, size_t n_replicates, const double *alpha0, double tol,
                            size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out);

/* msw_core_bootstrap and msw_core_bootstrap_dist solve the replicates on solver states of their own:
 * msw_core_gamma / msw_core_trace afterwards still describe the last msw_core_solve on the handle (the
 * reference writes the probabilities of the un-resampled estimate, src/mSWEEP.cpp:437-493). */

/* Only the resampling step: counts_out is (rep_end-rep_begin) x E uint32, bit-exact with
 * std::discrete_distribution<uint32_t> driven by std::mt19937_64(seed). */
int msw_core_resample_counts(msw_handle h, const uint32_t *ec_counts, size_t n_ecs,
                             int32_t seed, size_t bootstrap_count, size_t rep_begin,
                             size_t rep_end, uint32_t *counts_out);

/* ---- EC-sharded single solve over several GPUs --------------------------------------
 * The reference scales one solve only by OpenMP threads; rcgpar's MPI variant partitions the ECs
 * (columns) over ranks and all-reduces N, |g|^2 and the bound every iteration.
 * Here every rank holds a handle with a contiguous block of ECs (set_csr / build_likelihood /
 * set_dense_logl on the LOCAL ECs; all ranks pass the same groups and alpha0).  After
 * msw_core_set_comm, msw_core_solve / _prepare / _run take the local logc, exchange one scalar
 * and one (G + 4)-vector per iteration and return the SAME theta / iteration count on every rank.
 *   msw_comm_create_rccl : one process per GPU, RCCL over xGMI; `id` from msw_comm_unique_id on
 *                          rank 0, distributed by the caller (e.g. torch.distributed broadcast).
 *   msw_comm_create_local: the ranks are host threads of ONE process; out[] receives nranks
 *                          communicators (host-staged exchange, summed in rank order). */
typedef struct msw_comm *msw_comm_t;
int msw_comm_unique_id(unsigned char id_out[128]);
int msw_comm_create_rccl(const unsigned char id[128], int rank, int nranks, int device, msw_comm_t *out);
int msw_comm_create_local(int nranks, msw_comm_t *out);
/* msw_comm_create_shm: the ranks are PROCESSES of one host that meet in a POSIX shared-memory segment `name` ("/..."),
 * host-staged like the thread-ranks.  Test infrastructure for the process-per-rank paths on a box with one GPU (RCCL
 * refuses two ranks on one device): with MSWEEP_ALLREDUCE=peer the inboxes travel as hipIpc handles, as under RCCL. */
int msw_comm_create_shm(const char *name, int rank, int nranks, int device, msw_comm_t *out);
void msw_comm_destroy(msw_comm_t c);
/* ranks of the communicator and this rank's index (either pointer may be NULL) */
int msw_comm_size(msw_comm_t c, int *nranks, int *rank);
/* what RCCL itself reports for the communicator (ncclCommCount); 0 for an in-process communicator */
int msw_comm_rccl_count(msw_comm_t c, int *count);
/* recv[r * n .. (r + 1) * n) = rank r's send[0 .. n); host buffers, blocking (ncclAllGather through
 * device staging buffers).  The exchange step of the bootstrap (src/mSWEEP.cpp:513-517 stores every
 * replicate's abundances in one table, include/Sample.hpp:157). */
int msw_comm_allgather(msw_comm_t c, const double *send, size_t n, double *recv);
/* The per-iteration exchange of the sharded solve on host buffers (staged through device memory, blocking): ints[0..ni)
 * and reals[0..nr) are replaced by their sums over the ranks -- integers exactly, doubles in rank order, the same bits
 * on every rank.  Either part may be empty.  The transport is the communicator's: ncclAllReduce, the in-process
 * staging of thread-ranks, or -- MSWEEP_ALLREDUCE=peer in the environment when the communicator is created -- one
 * kernel that writes the message into every peer's inbox (msweep_amd/csrc/peer_comm.hpp).  Tests and timing. */
int msw_comm_allreduce(msw_comm_t c, uint64_t *ints, size_t ni, double *reals, size_t nr, int repeats,
                       double *ms_per_call);
/* comm == NULL detaches.  The communicator must outlive the solves that use it. */
int msw_core_set_comm(msw_handle h, msw_comm_t comm);
/* last error text of the msw_comm_* calls of this thread */
const char *msw_comm_last_error(void);

/* ---- pseudoalignment input (host code, no GPU) -------------------------
 * Replaces mSWEEP::Alignment::read + collapse (include/mSWEEP_alignment.hpp:97-215) for Themisto
 * plaintext files ("read_id target target ..." per line; one file per strand): reads -> sets of
 * targets, strands merged by intersection / union (--themisto-mode, :123-133), unaligned reads
 * dropped, reads keyed by the reference's 64-bit hash of their target set (:152-156) and collapsed
 * into equivalence classes in ascending hash order.  The export is what msw_core_build_likelihood
 * takes: ec_tptr[n_ecs + 1], ec_targets[n_hits] (ascending target ids of each EC's first read),
 * ec_counts[n_ecs] (Alignment::reads_in_ec, :220), plus ec_rptr[n_ecs + 1] / ec_reads[n_aligned]
 * (Alignment::reads_assigned_to_ec, :229: the read ids of every EC, ascending).  n_reads is the line
 * count of the last strand (Alignment::n_reads, :219).  Any output pointer may be NULL.
 * gzip-compressed files (Themisto --gzip-output; the reference opens its inputs through bxzstr, which detects
 * the compression by its magic bytes) are inflated with zlib by msw_alignment_read, and on the device by
 * msw_alignment_read_device (below: msw_inflate_info), with zlib behind it wherever the device's result cannot be
 * vouched for; bzip2 / xz files are refused by name.
 * The compact alignment-writer format is not supported (BitMagic): convert to plaintext. */
typedef struct msw_alignment *msw_alignment_t;
#define MSW_MERGE_INTERSECTION 0
#define MSW_MERGE_UNION 1
int msw_alignment_read(const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode,
                       msw_alignment_t *out);
int msw_alignment_shape(msw_alignment_t a, size_t *n_ecs, size_t *n_reads, size_t *n_hits, size_t *n_aligned);
int msw_alignment_export(msw_alignment_t a, uint64_t *ec_tptr, uint32_t *ec_targets, uint64_t *ec_counts,
                         uint64_t *ec_rptr, uint32_t *ec_reads);
/* The same five arrays WITHOUT a copy: pointers into the handle's own storage, valid until msw_alignment_destroy (round 5:
 * the export of cfg3's alignment -- 0.9 GB into freshly mapped memory, on one thread -- was a fifth of the whole
 * text-to-abundances time).  Any output pointer may be NULL.  msw_alignment_export copies on the reader's threads. */
int msw_alignment_view(msw_alignment_t a, const uint64_t **ec_tptr, const uint32_t **ec_targets, const uint64_t **ec_counts,
                       const uint64_t **ec_rptr, const uint32_t **ec_reads);
void msw_alignment_destroy(msw_alignment_t a);
/* The same reader ON THE DEVICE of handle h (round 5; msweep_amd/csrc/host_reader.inc): the text goes to device memory
 * as it is read and the parse, the rows by read id, the paired-end merge, the reference's hash, the sort and the
 * classes are kernels; the five arrays stay in device memory (msw_core_build_likelihood_aln consumes them there) and
 * msw_alignment_view / _export copy them out on first use.  Same outcome as msw_alignment_read, array for array.
 * Text the host parser would not take silently (anything but digits, blanks and line ends, ids beyond 32 bits,
 * target ids out of range) is handed to msw_alignment_read, whose result or error message stands
 * (msw_alignment_last_error / msw_last_error).
 * The alignment outlives every build from it: msw_core_build_likelihood_aln and msw_core_bin_reads_aln read its arrays
 * and never modify them, so one read serves every grouping column of the -i file (the contract is stated at
 * msw_core_build_likelihood_aln).  It is freed by msw_alignment_destroy only. */
int msw_alignment_read_device(msw_handle h, const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode,
                              msw_alignment_t *out);
/* gzip input of msw_alignment_read_device is inflated ON THE DEVICE (msweep_amd/csrc/host_inflate.inc): the compressed
 * bytes cross the link, a probe finds block starts inside the stream, the chunks between them are decoded side by side
 * against an unknown 32 KiB window, the windows are resolved in order and a second pass writes the text where the token
 * kernels read it.  The member's trailer is the guarantee: the device's text is used only when its CRC-32 and length are
 * the ones the file promises; otherwise -- and for several members, trailing bytes, a header the parser does not take,
 * a payload that does not fit, a stream with too few block starts for the device to pay -- zlib inflates the same file on the host, result and messages as before.
 * MSWEEP_HOST_INFLATE=1 in the environment (developer switch, read at the call) forces the host path.
 * BGZF files (bgzip, htslib: gzip files of many small members, each stating its compressed length in the 'BC' subfield
 * of its header and CRC-32 and length of at most 64 KiB of text in its trailer) take a shorter way
 * (msweep_amd/csrc/host_inflate_members.inc): headers and trailers are walked on the host, which gives every member's
 * payload and its offset in the text; one kernel decodes the members side by side, a wavefront each, and checks each
 * against its own trailer.  n_members counts them (the empty ones too); n_chunks = n_starts = n_members, chunk_bytes
 * = 0, payload_bytes = the sum of the members' DEFLATE bytes, write_ms = the decode with the check fused into it, and
 * probe_ms, window_ms, chain_ms, crc_ms = 0.  A file that starts with such a member and does not walk to its end member
 * by member (a plain member among them, a damaged length, trailing bytes) is the host's with the reason "header"; a
 * member that fails its check is the host's too (reasons 4, 5, 6).  Files of several members that do not declare their
 * lengths (cat a.gz b.gz) stay on the host: reason 6, as before.  On the single-member path and for plain files
 * n_members is 0. */
typedef struct msw_inflate_info {
  uint64_t payload_bytes, text_bytes;
  uint32_t chunk_bytes, n_chunks, n_starts;   /* chunks that begin at a block start the probe found (chunk 0 included) */
  int32_t on_device;                          /* 1: the bytes returned were inflated by the kernels and passed the trailer check */
  int32_t fallback_reason;                    /* 0 none; 1 forced, 2 header, 3 probe mismatch, 4 chunk status, 5 crc or length,
                                               * 6 trailing bytes, 7 memory, 8 long span (a stretch between two block
                                               * starts too long for one wavefront to pay: fixed-Huffman or stored
                                               * streams, one very long block) */
  uint32_t n_members;                         /* BGZF: the members walked and decoded one wavefront each; 0 otherwise
                                               * (fills what was padding: size and every other offset are unchanged) */
  double kernel_ms;                           /* events on the handle's stream: probe through CRC */
  double upload_ms;                           /* host clock: the compressed bytes to the device (files only) */
  double probe_ms, window_ms, chain_ms, write_ms, crc_ms; /* the parts of kernel_ms: probe, pass (a) with the scan, window
                                               * chain, pass (b), CRC -- each a pair of events directly around its
                                               * launches (a second strand shares the stream with the first one's token
                                               * kernels, which can fall inside a pair) */
} msw_inflate_info;
/* Test and diagnostic entry (the role msw_core_format_g6 has for the formatter): the text of the gzip bytes gz[0 .. n),
 * inflated by the kernels (chunk_bytes of payload per chunk; 0: the default, or MSWEEP_INFLATE_CHUNK) or, where their
 * result cannot be vouched for, by zlib (every member, as gzread reads a file).  *text_out is valid until the next
 * call; bytes that zlib rejects too fail the call with zlib's message. */
int msw_core_inflate_gzip(msw_handle h, const uint8_t *gz, size_t n, size_t chunk_bytes /* 0 = default */,
                          const uint8_t **text_out, size_t *len_out, msw_inflate_info *info);
/* One entry per file of the last msw_alignment_read_device on h, in the order of its paths (a plain file: all zero but
 * text_bytes): which path served each strand.  At most max_files entries are written; *n_files = how many there are. */
int msw_alignment_last_inflate(msw_handle h, msw_inflate_info *info, size_t max_files, size_t *n_files);

/* ---- --read-likelihood on the device (include/Likelihood.hpp:224-253) ------------------------------------------------
 * The file -- plain, gzip or BGZF: the same upload as msw_alignment_read_device, inflate included -- is parsed by kernels
 * (msweep_amd/csrc/likelihood_text_kernels.hpp, host_likelihood_file.inc) and the resident likelihood is built from the
 * staged matrix on by the code behind msw_core_set_dense_logl.  A file is SERVED or NOT SERVED.
 * Served (served = 1, reason = 0): the handle holds exactly the state msw_core_set_dense_logl would leave from the
 * host-parsed matrix of that file -- msw_core_get_dense_logl bit for bit, msw_core_layout_hash, msw_core_shape's nnz --,
 * re-expressed as CSR-of-ECs or kept dense alike.
 * Not served (served = 0, reason != 0): the call returns 0, whatever was resident before stays resident, and the caller
 * runs its own parser, whose result or message stands.  A non-zero return is a null argument or a HIP error only.
 * The device serves one grammar and judges no other text:
 *   every line is  count '\t' cell ('\t' cell){n_groups - 1} '\n'   (the last line may lack its '\n');
 *   count: 1 to 18 digits;  cell: inf, -inf, nan, -nan, or -?digits(.digits)?(e[+-]?digits)? of at most 24 bytes.
 * Any other byte ('\r', blanks, a '+' in front of a mantissa, upper case), a blank line, another column count, an empty
 * file, 2^32 - 1 or more lines, text and matrices that do not fit in free device memory: not served.  For the grammar
 * served, float(), std::stod and strtod agree on the value -- with one exception: a cell that rounds to a subnormal
 * (2.5e-320) is served with strtod's double, as float() reads it, although glibc sets ERANGE there and std::stod, hence
 * msweep_mini's host parser, throws on it.  Cells that one IEEE operation converts exactly (Clinger's case:
 * at most 2^53 as an integer, |decimal exponent| <= 22; msweep_amd/csrc/dec_parse.hpp) are converted by the kernels; the
 * others -- at most 65 536 per file, n_host_cells -- by strtod on the host, their bytes fetched from the device.
 * MSWEEP_HOST_LIKELIHOOD_FILE=1 in the environment (developer switch, read at the call): not served, reason forced. */
#define MSW_LIKFILE_FORCED 1      /* the developer switch */
#define MSW_LIKFILE_OPEN 2        /* the file cannot be opened or read (inflate errors included) */
#define MSW_LIKFILE_BAD_BYTE 3    /* a byte outside the grammar */
#define MSW_LIKFILE_BAD_TOKEN 4   /* a count or cell the grammar does not have; a cell of more than 24 bytes */
#define MSW_LIKFILE_COLUMNS 5     /* a line without n_groups + 1 columns (blank lines, doubled tabs, n_groups = 0) */
#define MSW_LIKFILE_EMPTY 6       /* no text */
#define MSW_LIKFILE_HOST_CELLS 7  /* more than 65 536 cells for the host's strtod */
#define MSW_LIKFILE_RANGE 8       /* strtod reports ERANGE and returns an infinity or zero (1e400, 1e-400) */
#define MSW_LIKFILE_MEMORY 9      /* text plus matrices do not fit in free device memory */
#define MSW_LIKFILE_LINES 10      /* 2^32 - 1 or more lines */
typedef struct msw_likfile_info {
  uint64_t text_bytes, n_ecs, n_host_cells;   /* the (inflated) text; lines; cells converted on the host */
  int32_t served, reason;                     /* reason: 0 or MSW_LIKFILE_* */
  double upload_ms, kernel_ms;                /* host clock: the text to the device (inflate included); events: pass 1 through the transpose */
  msw_inflate_info inflate;                   /* the file's entry of msw_alignment_last_inflate (a plain file: text_bytes only) */
} msw_likfile_info;
int msw_core_set_dense_logl_file(msw_handle h, const char *path, size_t n_groups, msw_likfile_info *info);
/* test / diagnostic entry: plain text in host memory */
int msw_core_set_dense_logl_text(msw_handle h, const char *text, size_t n, size_t n_groups, msw_likfile_info *info);
/* first column of the last served file: the read counts of its n_ecs lines */
int msw_core_likfile_counts(msw_handle h, uint64_t *counts_out, size_t n_ecs);

/* ---- --extract-reads: the binned reads themselves, from the FASTQ files (docs/pipeline.md:59-64 runs a second tool,
 * `mGEMS extract`, for this step) ---------------------------------------------------------------------------------------
 * A read file -- plain, gzip or BGZF: the same upload as msw_alignment_read_device, inflate included -- becomes resident
 * on h's device with an index of its records (msweep_amd/csrc/fastq_kernels.hpp, host_fastq.inc); a selection of read ids
 * -- a bin of msw_core_bin_reads -- is then gathered there, and its records come back as plain bytes or inside the
 * handle's open gzip stream, where only compressed bytes cross the link.
 * The grammar is the strict four-line one: a record is four lines, the first begins with '@', the third with '+', the
 * second and the fourth have the same length (a '\r' in front of the '\n' counts on both), the line count is a multiple
 * of 4; a last line without '\n' counts as a line.  Lines are counted, '@' is never searched for.  Read id i is the
 * i-th record of the file, from 0; ids are below 2^32.  One text is resident per file, whole.
 * msw_fastq_open    reason / bad_record: 0, or why the file is outside the grammar (1 line count, 2 no '@', 3 no '+',
 *                   4 lengths differ) and the 0-based number of the smallest offending record; the call then fails with a
 *                   message that names the record from 1.  A text and index that do not fit in free device memory fail
 *                   with a message naming the bytes.  index_ms / upload_ms: host clock around the index kernels / the
 *                   upload (inflate included); inflate: the file's entry as msw_alignment_last_inflate reports one.
 *                   The handle stays usable after every failure.  The object belongs to h: close it before
 *                   msw_core_destroy(h).
 * msw_fastq_select  replaces the current selection by the records `ids` names: sorted ascending, every id once (file
 *                   order).  n == 0 is valid.  An id >= n_records fails the call, which names it and the record count,
 *                   and leaves the selection as it was.  *n_selected_out: the distinct ids; *bytes_out: their records' bytes.
 * msw_fastq_next    the next whole records of the selection, at most max_bytes (1 MiB ... 1 GiB) of them, copied verbatim:
 *                   *out points into a pinned buffer of the handle, valid until the next msw_fastq_* call on it;
 *                   *len_out == 0: the selection is exhausted.  Every piece ends at a record end; a record longer than
 *                   max_bytes fails the call (the selection stays where it was).
 * msw_fastq_next_gzip  the same inside the handle's open gzip stream (msw_core_gzip_begin ... _end): returns the bytes to
 *                   append to the file, as msw_core_text_block_gzip does; *text_len_out (may be NULL): the plain length.
 * msw_fastq_last_timing  measurement hook (tools/extract_timing.py): device time of the gather kernel over the pieces since
 *                   the last msw_fastq_select (events on the handle's stream; copies and the gzip kernels are not in it)
 *                   and the bytes it wrote.
 * MSWEEP_HOST_EXTRACT=1 in the environment at msw_fastq_open (developer switch): the file is read and inflated by zlib on
 * the host and indexed, validated and gathered by plain host loops (msweep_amd/csrc/fastq_host.hpp) behind the same calls,
 * with the same messages -- the second tool's method, the other side of the A/B and of the tests; msw_fastq_last_timing
 * then reports the host clock of the gather loop. */
typedef struct msw_fastq *msw_fastq_t;
typedef struct msw_fastq_info {
  uint64_t n_records, text_bytes;
  int32_t reason;
  uint64_t bad_record;
  msw_inflate_info inflate;
  double index_ms, upload_ms;
} msw_fastq_info;
int msw_fastq_open(msw_handle h, const char *path, msw_fastq_t *out, msw_fastq_info *info);
int msw_fastq_select(msw_handle h, msw_fastq_t fq, const uint32_t *ids, size_t n, uint64_t *n_selected_out,
                     uint64_t *bytes_out);
int msw_fastq_next(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out);
int msw_fastq_next_gzip(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out,
                        size_t *text_len_out);
int msw_fastq_last_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out);
void msw_fastq_close(msw_fastq_t fq);
/* 1: the handle's arrays are device-resident (msw_alignment_read_device served the text with its kernels); 0: host
 * arrays (msw_alignment_read, or the host parser behind the device entry). */
int msw_alignment_on_device(msw_alignment_t a);
/* msw_alignment_read_device keeps its device temporaries (~5 bytes per byte of text) on the handle between calls: a
 * repeated read allocates nothing, and nothing is freed in front of the likelihood build (memory given back is scrubbed
 * before it is handed out again: 0.2 s at 10 M reads).  msw_core_trim gives them back; msw_core_destroy does too. */
int msw_core_trim(msw_handle h);
/* msw_core_build_likelihood on an alignment handle: arrays resident on h's device are read where they lie (no copy
 * through the host); any other handle goes through its host arrays.  ec_counts = the classes' read counts.
 * The contract of repeated builds (the grouping loop of src/mSWEEP.cpp:282: one read, one build per column of -i):
 *   - an alignment may be built from any number of times, with any target-to-group map over the same n_targets (another
 *     n_groups, other sizes, another --min-hits mask, in any order);
 *   - each build REPLACES the resident likelihood and everything derived from it: the solver state (no solution, nothing
 *     prepared), the slot tables and the record encoding, the guard lists, the trace, gamma and the EC permutation
 *     behind its blocks.  Two things are kept because they do not depend on the likelihood: the dynamic-LDS limit
 *     granted per sweep instantiation (only ever raised; each launch passes the size its own layout needs) and the
 *     bootstrap's cumulative table (made from the read counts alone; reused while they are the same);
 *   - the alignment's arrays are not modified: a build after K others reads what the first one read;
 *   - msw_core_bin_reads_aln, msw_core_gamma*, msw_core_trace and msw_core_text_block* refer to the LATEST build and its
 *     latest solve (a call that needs a solve fails until that build has been solved).
 * A build on a used handle gives, bit for bit, what the same build gives on a fresh one (tests/test_gpu_groupings.py). */
int msw_core_build_likelihood_aln(msw_handle h, msw_alignment_t a, const uint32_t *target_group, size_t n_targets,
                                  const uint64_t *group_sizes, size_t n_groups, double q, double e,
                                  double zero_inflation, size_t min_hits, size_t *n_groups_out, uint8_t *mask_out,
                                  double *logc_out);
/* An alignment RESTRICTED to a set of reads and a set of target sequences, collapsed into equivalence classes again
 * (msweep_amd/csrc/host_subset.inc, subset_kernels.hpp).  The whole contract:
 *   *out is, array for array (ec_tptr, ec_targets, ec_counts, ec_rptr, ec_reads and the four numbers of
 *   msw_alignment_shape), the alignment of the single-strand plaintext text with *n_targets_out = the number of non-zero
 *   entries of keep_target[a's n_targets] target sequences that holds one line per entry of read_ids: the read id as it is
 *   (ids are NOT renumbered), followed by those targets of the read's class in `a` that keep_target keeps, each written as
 *   its rank among the kept targets (kept sequences are renumbered 0 .. n_keep - 1 in ascending order).  A read that is in
 *   no class of `a`, or whose targets are all dropped, gives a bare id.
 * Hence n_reads = n_ids; unaligned reads are dropped; classes stand in ascending order of the reference's 64-bit hash over
 * the RENUMBERED ids, reads with equal hash share a class, a class's target list is that of its smallest read id, read ids
 * ascend inside a class.  Classes of `a` that differed only in dropped targets fall together; a class of which no read is
 * selected, or which loses every target, is gone.
 * EVERY selected read takes part, whatever its id: this is the text as the reader's rule (and the pure-Python mirror,
 * msweep_amd/alignment.py) reads it.  msw_alignment_read itself leaves out read ids at or beyond the text's LINE COUNT
 * (its guard against a malformed line sizing the tables; a Themisto file numbers its reads 0 .. lines - 1), so on a text
 * of n_ids lines it returns the same arrays exactly when every selected id is below n_ids, and otherwise when the text is
 * given one bare line for every id that is not selected, up to the largest one (tests/test_alignment_subset_cpu.py).
 * The output is an ordinary alignment handle: it can be built from, binned, assigned and subset again, and is freed by
 * msw_alignment_destroy.  `a` is not modified.
 * Refused (non-zero, msw_last_error(h); msw_last_error(NULL) when h is NULL): a read id listed twice (the message names
 * the SMALLEST such id, whatever the order of read_ids and of the threads); keep_target all zero; `a` resident on another
 * device than h's; a NULL h with a device-resident `a`.  n_ids == 0, and a selection in which no read keeps a target, are
 * valid and give an alignment of 0 classes.
 * A device-resident `a` is served by kernels on h's stream, its result stays resident: the kept targets are ranked by a
 * scan, every class's list is filtered, renumbered and hashed ONCE, the selection becomes a bitmap over the read ids, the
 * selected reads carry their class's hash through a stable radix sort, and the classes are taken as the reader takes them.
 * No atomic decides an order: two calls give the same bytes.  Device memory: O(largest selected id + classes and hits of
 * `a` + the output), temporaries from the handle's reader pool (msw_core_trim); an allocation that fails is an error that
 * names the bytes, never a fall back.  A host-resident `a` (msw_alignment_read, or the host parser behind the device
 * entry) is served by plain loops on the host, h may be NULL and no GPU is touched.
 * MSWEEP_HOST_SUBSET=1 in the environment (developer switch, read at the call): the host loops also for a resident `a`.
 * This restricts the pseudoalignment against the FULL index; it is not a pseudoalignment against an index of the kept
 * sequences alone. */
int msw_alignment_subset(msw_handle h, msw_alignment_t a, const uint32_t *read_ids, size_t n_ids, const uint8_t *keep_target,
                         msw_alignment_t *out, size_t *n_targets_out);
/* error text of the last failed msw_alignment_read of this thread (the reference's messages) */
const char *msw_alignment_last_error(void);

/* ---- measurement hooks (used by bench.py; no effect on results) ---------------------- */
/* Device time (ms, HIP events on the solve stream) and launch counts of the dominant
 * kernels during the last solve: pass A (gradient norm sweep) and pass B (softmax /
 * column-sum / ELBO sweep). */
typedef struct msw_timing {
  double solve_ms;       /* whole solve loop, events on the solve stream */
  double passA_ms;       /* summed over launches (only when profiling is enabled) */
  double passB_ms;
  uint64_t passA_launches;
  uint64_t passB_launches;
  uint64_t iters;
  uint64_t bytes_passA;  /* algorithmic bytes per launch */
  uint64_t bytes_passB;
  double collective_ms;  /* EC-sharded solve, profiling enabled: the all-reduces of the solve (one scalar after pass A,
                          * one (3 G + 4)-word vector after pass B, per iteration) with the small kernels that pack
                          * them, summed over the launches; events on the solve stream.  0 without a communicator. */
  uint64_t collectives;  /* how many */
  uint64_t em_float_kernels; /* 1: the last solve was an EM run under MSW_PREC_FLOAT served by the fp32 kernels */
} msw_timing;
int msw_core_set_profiling(msw_handle h, int enabled);
int msw_core_last_timing(msw_handle h, msw_timing *out);
/* Host wall-clock split of the last msw_core_bootstrap / msw_core_bootstrap_dist on the handle (bench.py's
 * cfg4 leg): where a rank's time went.  No reference counterpart. */
typedef struct msw_bootstrap_timing {
  double table_ms;      /* init_bootstrap (src/BootstrapSample.cpp:33-44): cumulative table on the host + upload */
  double solve_ms;      /* this rank's block of replicates: seek / jump-ahead, resampling (under the solves), solves */
  double gather_ms;     /* msw_core_bootstrap_dist: the all-gather, waiting for the slowest rank included */
  uint64_t replicates;  /* solved on this rank */
  uint64_t iterations;  /* summed over them */
  uint64_t table_reused; /* 1: the call brought the EC counts of the resident table again (compared, not rebuilt) */
} msw_bootstrap_timing;
int msw_core_last_bootstrap_timing(msw_handle h, msw_bootstrap_timing *out);
/* Reporting (tests, diagnostics): how many equivalence classes pass B has evaluated through the cancellation guard
 * (Z formed over every group instead of background + listed cells) since the likelihood became
 * resident on this handle, summed over the iterations.  No reference counterpart. */
int msw_core_guarded_visits(msw_handle h, uint64_t *out);
/* Measurement only (bench.py's roofline object): the streaming rates this device reaches on n_bytes of HBM --
 * a read-only 16-byte-load sweep (the shape of the sweeps' record stream) and the triad a = b + 3 c -- best of
 * `reps` launches after two warm-up launches, in GB/s (1e9).  SURVEY.md 8(d): the practical ceiling beside the
 * 8 TB/s specification.  No reference counterpart. */
int msw_core_hbm_stream_rates(msw_handle h, size_t n_bytes, int reps, double *read_gbs, double *triad_gbs);
/* fixed-iteration mode for benchmarking: run exactly max_iters iterations (tol ignored) */
int msw_core_set_fixed_iters(msw_handle h, int enabled);
/* n_iters MORE iterations of the fixed-iteration RCG solve that last ran on the handle (msw_core_run in
 * fixed-iteration mode): the optimiser state carries on where it stood.  bench.py's W warm-up steps are
 * msw_core_run(W), its K timed steps msw_core_continue(K).  *iters_out = total iterations so far. */
int msw_core_continue(msw_handle h, size_t n_iters, double *theta_out, size_t *iters_out, double *bound_out);

#ifdef __cplusplus
}
#endif
#endif
