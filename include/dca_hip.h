/* dca_hip.h -- C ABI of the MI355X-native DCA compute core (libdca_hip.so).
 *
 * Plain C: opaque handle, raw pointers and sizes, int status codes.  No torch / C++
 * types cross this boundary and nothing throws across it.  Host buffers are
 * caller-owned, C-contiguous.  A context owns one HIP device and one HIP stream;
 * calls on one context are serialised by the caller, different contexts are
 * independent (no globals except the thread-local error string).
 *
 * Each entry names the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef DCA_HIP_H
#define DCA_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status codes */
#define DCA_OK 0
#define DCA_ERR_ARG (-1)        /* invalid argument / call order */
#define DCA_ERR_IO (-2)         /* cannot open MSA file (reference: throws, plmdca_numerics.cpp:743-746) */
#define DCA_ERR_RESIDUE (-3)    /* character outside the reference's table or short line (reference: std::out_of_range, :752) */
#define DCA_ERR_NOMEM (-4)
#define DCA_ERR_HIP (-5)        /* HIP runtime error; text in dca_last_error() */
#define DCA_ERR_NO_DEVICE (-6)  /* no usable gfx950 device: the product never falls back to a CPU path */
#define DCA_ERR_NOT_SPD (-7)    /* correlation matrix not positive definite (reference: numpy LinAlgError, meanfield_dca.py:542-548) */
#define DCA_ERR_STATE (-8)      /* required earlier stage has not been run */

#define DCA_BIOMOLECULE_PROTEIN 1 /* q = 21, plmdca.py:57 */
#define DCA_BIOMOLECULE_RNA 2     /* q = 5 */

#define DCA_F32 32
#define DCA_F64 64

/* carry_mode of dca_plm_configure */
#define DCA_CARRY_EXACT 0   /* mathematically exact pseudolikelihood gradient (opt-in) */
#define DCA_CARRY_CHUNKED 1 /* reference semantics (plmdca_numerics.cpp:492-530 carry-over), chunk-parallel scan with warm-up */
#define DCA_CARRY_SERIAL 2  /* reference semantics, one strictly serial chain per site (slow; checking mode) */

typedef struct dca_ctx dca_ctx;

const char* dca_last_error(void);
int dca_device_count(void);
const char* dca_version(void);
/* Device blocks of 1 MiB and more are kept in a process-wide cache when a context releases them and are handed to
 * later contexts (DCA_POOL_MAX_BYTES, default 64 GiB per process).  This returns them to the driver; result: bytes released. */
size_t dca_release_cached_memory(void);
/* Device blocks the library has allocated and not yet released, of any size, over all contexts of the process (a block in
 * the cache above is not in use). */
size_t dca_device_blocks_in_use(void);

/* ------------------------------------------------------------------ drop-in FFI
 * Same symbols, signatures and meaning as the reference's ctypes boundary
 * (pydca/plmdca/plmdcaBackend.cpp:151-156 and :204; bound in pydca/plmdca/plmdca.py:79-89).
 * Returns a malloc()'d block of L*q + L(L-1)/2*q*q floats, or NULL on any error
 * (reason in dca_last_error()); release it with freeFieldsAndCouplings (free()).
 * num_threads is accepted and ignored (the work runs on the GPU). */
float* plmdcaBackend(unsigned short biomolecule, unsigned short num_site_states, const char* msa_file,
                     unsigned int seqs_len, float seqid, float lambda_h, float lambda_J,
                     unsigned int max_iteration, unsigned int num_threads, bool verbose);
void freeFieldsAndCouplings(void* h_and_J);

/* ------------------------------------------------------------------ MSA input
 * dca_read_msa: PlmDCA::readSequencesFromFile (plmdca_numerics.cpp:685-767): one
 * sequence per non-empty, non-'>' line, first L characters, 0-based codes with
 * gap = q-1, exact duplicates dropped keeping the first occurrence.
 * Returns the number of unique rows (>=0) or a DCA_ERR_*; raw_count (optional)
 * receives the number of sequence lines read. */
int dca_read_msa(const char* path, int biomolecule, int L, uint8_t* out, int capacity, int* raw_count);
int dca_count_msa_lines(const char* path);
/* The same reader in ONE pass over the file (what plmdcaBackend itself uses): allocates *rows (unique rows x L bytes; release
 * with dca_host_free) and returns the number of unique rows.  The two-call form above opens the file twice, which a pipe
 * does not survive. */
int dca_read_msa_alloc(const char* path, int biomolecule, int L, uint8_t** rows, int* raw_count);

/* The mfDCA path's FASTA reader, pydca/fasta_reader/fasta_reader.py:81-163 (there through Biopython): multi-line
 * records, upper-casing, every character outside the alphabet is the gap state (:138-149), exact duplicates dropped
 * keeping the first occurrence (:153).  Codes are 0-based with gap = q-1 (the reference's Python states minus one).
 * dca_fasta_shape: number of records with residues and their common length (DCA_ERR_ARG if lengths differ).
 * dca_read_fasta: out = capacity x L bytes; returns the number of unique rows; raw_count = records read.  Files with
 * non-ASCII bytes return DCA_ERR_RESIDUE (the Python side then reads them in text mode itself). */
int dca_fasta_shape(const char* path, int* n_records, int* L_out);
int dca_read_fasta(const char* path, int biomolecule, int L, uint8_t* out, int capacity, int* raw_count);
/* The same in ONE pass over the file: the reader allocates *rows (unique rows x *L_out bytes; release with
 * dca_host_free) and returns the number of unique rows. */
int dca_read_fasta_alloc(const char* path, int biomolecule, uint8_t** rows, int* L_out, int* raw_count);
void dca_host_free(void* p);

/* Query sequences for the energy entries (no reference counterpart): record k is seqs[offsets[k] .. offsets[k+1]) (offsets
 * has nseq + 1 entries), encoded into out (nseq x L bytes, 0-based codes, gap = q-1) in input order, nothing de-duplicated.
 * table 0: the residue table of dca_read_msa -- a character that reader rejects is DCA_ERR_RESIDUE; table 1: the table of
 * dca_read_fasta -- every unknown character is the gap state.  A record of a length other than L is DCA_ERR_ARG.  On either
 * error *bad_record (may be NULL) receives the 0-based index of the offending record (-1 otherwise). */
int dca_encode_sequences(const char* seqs, const int* offsets, int nseq, int biomolecule, int table /* 0: plm, 1: mf */,
                         int L, uint8_t* out, int* bad_record);

/* ------------------------------------------------------------------ reference-sequence back-mapping (host)
 * Local pairwise alignment, Smith-Waterman with affine gaps (a gap of length n costs
 * gap_open + (n-1)*gap_extend), standing in for Bio.pairwise2.align.localds as called by
 * SequenceBackmapper.align_pairs_local (sequence_backmapper.py:186-230; biopython 1.74 is a
 * dependency outside the reference tree).  sub: 26 x 26 substitution scores indexed by
 * (letter - 'A').  dca_sw_scores is the search loop of find_matching_seqs_from_alignment
 * (:233-283): best local score of ref against nseq sequences stored back to back in seqs,
 * sequence k = seqs[offsets[k] .. offsets[k+1]).  dca_sw_align returns one optimal alignment:
 * the aligned region (with '-') in aligned_a / aligned_b (capacity la + lb + 1 each) and the
 * 0-based start of the region in each sequence. */
int dca_sw_scores(const char* ref, int lref, const char* seqs, const int* offsets, int nseq, const int* sub,
                  int gap_open, int gap_extend, int* scores_out);
int dca_sw_align(const char* a, int la, const char* b, int lb, const int* sub, int gap_open, int gap_extend,
                 int* score_out, int* start_a, int* start_b, char* aligned_a, char* aligned_b, int* aligned_len);

/* ------------------------------------------------------------------ profile alignment (device)
 * Aligns n sequences to a profile of Lp columns over A codes, one wave64 lane per sequence.  Integers only:
 *     D[i][j] = max(D[i-1][j] + del_extend[i], H[i-1][j] + del_open[i])         column i deleted
 *     I[i][j] = max(I[i][j-1] + ins_extend,    H[i][j-1] + ins_open)            residue j inserted
 *     H[i][j] = max(H[i-1][j-1] + match[i][s_j], D[i][j], I[i][j])              DCA_ALIGN_LOCAL: also 0
 * match: Lp x A; del_open, del_extend: Lp, each <= 0; ins_open, ins_extend <= 0.  seqs: codes < A, sequence k =
 * seqs[offsets[k] .. offsets[k+1]), 0 .. 32767 residues.  DCA_ALIGN_LOCAL is Smith-Waterman (score: the maximum over all cells,
 * the end cell the first maximum in row-major order, i outer); DCA_ALIGN_GLOCAL accounts for every column and lets the query
 * overhang for free (H[0][j] = 0, H[i][0] = D[i][0] = del_open[1] + sum_{k=2..i} del_extend[k]; score: max_j H[Lp][j] at the
 * smallest such j).  The traceback is dca_sw_align's: in H the diagonal, then D, then I (local: stop at H = 0); in D or I back
 * to H whenever "open" is co-optimal with "extend".  residue_at_out (n x Lp, or NULL for scores only): the 0-based index in
 * the sequence of the residue matched to column i, or -1.  Needs a context, no alignment.  DCA_ERR_ARG: Lp outside 1..8192, A
 * outside 2..32, a positive penalty, (max|match| + max|penalty|) * (Lp + 32767) >= 2^28, a sequence longer than 32767, a code
 * >= A (the message names the record).  The scratch of a call stays within 1 GiB by running the queries in passes;
 * DCA_ALIGN_PASS caps the queries per pass; the results do not depend on the split.
 * dca_profile_align_last_scratch: bytes of edge columns and pointer bits the largest pass of the context's last call took.
 * dca_sw_scores_device: dca_sw_scores on the device, the same integers -- the profile match[i][b] = sub[ref_i][b] over 26
 * letters plus "other" (-4 against everything), local mode, scores only.  lref 1..8192, gap penalties <= 0. */
#define DCA_ALIGN_LOCAL 0
#define DCA_ALIGN_GLOCAL 1
int dca_profile_align(dca_ctx* ctx, const int32_t* match, int Lp, int A, const int32_t* del_open, const int32_t* del_extend,
                      int ins_open, int ins_extend, int mode, const uint8_t* seqs, const int64_t* offsets, int n,
                      int32_t* score_out /* n */, int32_t* residue_at_out /* n*Lp or NULL */);
int dca_profile_align_last_scratch(dca_ctx* ctx, unsigned long long* bytes_out);
/* the context's alignment as dca_set_msa received it: N x L codes (what a profile is built from) */
int dca_get_msa(dca_ctx* ctx, uint8_t* out);
int dca_sw_scores_device(dca_ctx* ctx, const char* ref, int lref, const char* seqs, const int* offsets, int nseq,
                         const int* sub, int gap_open, int gap_extend, int* scores_out);

/* ------------------------------------------------------------------ context */
int dca_create(dca_ctx** out, int device, int precision /* DCA_F32 | DCA_F64 */);
void dca_destroy(dca_ctx* ctx);
/* X: N x L, 0-based codes < q, gap = q-1 (the C++ coding; the Python mfDCA layer
 * converts from the reference's 1-based coding).  Copies to the device; the range of the codes is checked there (a code >= q
 * is DCA_ERR_ARG with the element's position, and the context then holds NO alignment -- not the one it held before).
 * N >= 1, L >= 1, 2 <= q <= 32; the model entries (plm, mf, ar) need L >= 2 and answer DCA_ERR_STATE on a one-site alignment. */
int dca_set_msa(dca_ctx* ctx, const uint8_t* X, int N, int L, int q);

/* Sequence weights: PlmDCA::computeSeqsWeight (plmdca_numerics.cpp:611-671) when
 * compare_precision == DCA_F32 ((float)ident/(float)L > (float)seqid) and
 * msa_numerics.compute_sequences_weight (meanfield_dca/msa_numerics.py:13-50) when
 * DCA_F64.  Integer-exact. */
int dca_compute_weights(dca_ctx* ctx, double seqid, int compare_precision);
int dca_set_weights(dca_ctx* ctx, const double* w);           /* externally computed weights */
int dca_get_weights(dca_ctx* ctx, double* w_out);             /* N values: 1/count */
int dca_get_weight_counts(dca_ctx* ctx, uint32_t* counts_out);/* N values (after dca_compute_weights) */
/* Measurement aid (bench.py's roofline of the weights kernel): the integer work the last dca_compute_weights launch really
 * issued -- out[0] = wave x 32-site groups compared (each 16 pairs per lane x (planes xor/or + 1 popcount-add) VALU
 * instructions), out[1] = the same count without the exact early exit, out[2] = bit planes per group (5 or 3). */
int dca_weights_work(dca_ctx* ctx, uint64_t* out3);
int dca_get_meff(dca_ctx* ctx, double* meff_out);

/* ------------------------------------------------------------------ plmDCA
 * dca_plm_configure fixes lambda_h / lambda_J (PlmDCA ctor, plmdca_numerics.cpp:17-48),
 * the carry mode and the scan geometry (chunk sequences per independent scan, warm-up
 * steps; 0 = defaults 128 / 40).  halo = number of leading sequences of this context's
 * MSA that only warm up the scan and do not contribute to fx/g (used by sequence
 * sharding; 0 otherwise).  add_regulariser = 0 on every shard except one. */
int dca_plm_configure(dca_ctx* ctx, double lambda_h, double lambda_J, int carry_mode,
                      int chunk, int warmup, int halo, int add_regulariser);
size_t dca_plm_num_params(int L, int q);
/* Frees the context's plmDCA state (x, g, the N x L q logit / residual tables, optimiser vectors); alignment, weights and
 * communicator stay.  The next dca_plm_configure starts afresh.  For callers that configure a context only to take the
 * initial point from it (the per-rank set-up of a multi-GPU run) -- no counterpart in the reference, whose PlmDCA object owns
 * nothing between plmdcaBackend calls (plmdcaBackend.cpp:151-204). */
int dca_plm_release(dca_ctx* ctx);
/* x <- initial fields/couplings: PlmDCA::initFieldsAndCouplings (plmdca_numerics.cpp:207-249) */
int dca_plm_init_x(dca_ctx* ctx);
int dca_plm_set_x(dca_ctx* ctx, const void* x, int dtype);
int dca_plm_get_x(dca_ctx* ctx, void* x_out, int dtype);
/* fx, g at the context's current x: PlmDCA::gradient (plmdca_numerics.cpp:436-607) */
int dca_plm_gradient(dca_ctx* ctx, double* fx_out);
int dca_plm_get_g(dca_ctx* ctx, void* g_out, int dtype);

/* ------------------------------------------------------------------ native collectives (RCCL over xGMI)
 * One process per GPU; every context owns one RCCL communicator whose collectives are enqueued on the context's own
 * stream, in place on the library's buffers: with it an objective evaluation has no host callback and no device
 * synchronisation around its exchange step.  librccl.so is opened with dlopen: rccl_path if given, else $DCA_RCCL_PATH,
 * else the librccl that lies next to the libamdhip64 this library is bound to (RCCL must run on the same HIP runtime:
 * it receives this library's stream and pointers; a process that also holds PyTorch can contain two HIP runtimes).
 *   rank 0:      dca_comm_unique_id(path, id)           128 bytes; hand them to every rank (store, MPI, file ...)
 *   every rank:  dca_comm_init(ctx, path, id, world, rank)   collective: returns when all ranks have called it
 * No reference counterpart (pydca is single-process); the partition is the one BASELINE.json's north_star names. */
int dca_comm_unique_id(const char* rccl_path, void* id128);
int dca_comm_init(dca_ctx* ctx, const char* rccl_path, const void* id128, int world, int rank);
int dca_comm_destroy(dca_ctx* ctx);
/* For a WATCHDOG thread (the only entry point that may be called while another thread is inside a call on the same context): a
 * peer rank has died; ncclCommAbort releases the communicator and makes the collectives that wait for the peer fail, so the
 * driving thread's call returns an error instead of hanging.  DCA_ERR_STATE if the collective library has no ncclCommAbort. */
int dca_comm_abort(dca_ctx* ctx);
/* world size and rank as the communicator itself reports them (ncclCommCount / ncclCommUserRank): a launcher asserts with
 * it that its N processes form ONE communicator of N ranks.  dca_comm_init / dca_comm_destroy answer DCA_ERR_STATE, and
 * change nothing, while an optimisation whose vectors are cut for the current communicator is in progress. */
int dca_comm_info(dca_ctx* ctx, int* world, int* rank);
/* Small host-side exchange over the context's communicator: every rank hands in n doubles, every rank receives all world * n of
 * them in rank order (timings, status flags of a start-up protocol; collective, synchronises the context's stream). */
int dca_comm_allgather_host(dca_ctx* ctx, const double* mine, int n, double* all);

/* Exchange step of the sharded plmDCA evaluation through the context's communicator (after dca_plm_configure):
 *   mode 1: all-reduce(sum) of the gradient and of fx after every evaluation, optimiser vectors replicated;
 *   mode 2: sharded optimiser vectors -- reduce-scatter(g) per evaluation, all-gather(x) per step, scalar all-reduces
 *           (the scheme of dca_plm_set_vector_sharding; rank / world are the communicator's);
 *   mode 3: mode 2 with the two vector collectives as a DIRECT EXCHANGE -- grouped ncclSend / ncclRecv of slice j
 *           straight to rank j (every xGMI link of the mesh busy at once) and a local sum of the received pieces in
 *           rank order -- for topologies / sizes where RCCL would run its reduce-scatter and all-gather as rings;
 *   mode 0: off.  Replaces any hook set with dca_plm_set_reduce_hook / dca_plm_set_vector_sharding. */
int dca_plm_set_native_comm(dca_ctx* ctx, int mode);

/* Column-strip decomposition of the plmDCA evaluation over the context's communicator (exchange mode 4; instead of
 * dca_plm_configure + dca_plm_set_native_comm).  The context holds the WHOLE alignment and its weights, like a
 * single-GPU one; rank r of `world` holds the columns of sites [L r / world, L (r+1) / world) of the coupling table and of
 * every per-sequence array, walks all sequences for them -- logits, carry scan and scatter stay local, no halo -- and owns
 * the packed parameters of the pairs (i, j), i < j, whose first site it holds (rank 0 the fields too), with their share
 * of the L-BFGS vectors.  Per evaluation two grouped point-to-point exchanges cross the wires: the couplings a rank's
 * columns need from LOWER ranks (and its sites' fields from rank 0) before the table is expanded, and the rows of the
 * gradient table that belong to the sites of lower ranks (and the field gradients for rank 0) before the fold --
 * (L q)^2 / 2 x (1 - 1/world) elements each way summed over the node, against 2 x (world - 1) x P for the sequence-sharded
 * schemes (config D, 8 ranks: 2 x 193 MB against 2 x 1.5 GB), as all-to-all traffic over every xGMI link at once.
 * This is the reference's own parallel axis (its OpenMP loop runs over sites, plmdca_numerics.cpp:490).
 * dca_plm_get_x / _get_g / _scores are collective in this mode (every rank calls them). */
int dca_plm_configure_strips(dca_ctx* ctx, double lambda_h, double lambda_J, int carry_mode, int chunk, int warmup);

/* mfDCA pair counts summed over the shards through the communicator (instead of dca_mf_set_reduce_hook). */
int dca_mf_set_native_comm(dca_ctx* ctx, int on);
/* The decomposition behind MeanFieldDCA(devices = ...): every rank holds the WHOLE alignment and all weights (tens of MB) and
 * counts the sequences [first, first + count) only; with dca_mf_set_native_comm(ctx, 1) the raw pair counts of the windows are
 * summed over the ranks (Meff is the global one everywhere).  Frequencies, correlation matrix, inverse and scores then run as
 * on one GPU on every rank that asks for them; a rank that gives its communicator back afterwards keeps the summed counts.
 * count < 0: the whole alignment again.  (The reference has one process and no counterpart.) */
int dca_mf_set_row_window(dca_ctx* ctx, int first, int count);

/* Sequence weights with the N^2 L / 2 comparisons divided over the ranks (every rank holds the whole alignment --
 * tens of MB -- and counts every world-th tile pair of the upper triangle of the identity matrix; the symmetric
 * half-loop of plmdca_numerics.cpp:646-666, split evenly), then ONE all-reduce(sum) of the N integer counts
 * through the communicator: exact, the same counts on every rank as dca_compute_weights gives. */
int dca_compute_weights_sharded(dca_ctx* ctx, double seqid, int compare_precision);

/* The same split without a communicator: part `part` of `parts` of the comparisons -> partial counts (host array of N,
 * optional); the caller sums the parts by any means and hands the totals back with dca_set_weight_counts. */
int dca_weights_partial_counts(dca_ctx* ctx, double seqid, int compare_precision, int part, int parts, uint32_t* counts_out);
int dca_set_weight_counts(dca_ctx* ctx, const uint32_t* counts);

/* Optional reduction hook for sequence sharding: called after the local data term is
 * on the device, before the optimiser sees it.  g_dev/fx_dev are DEVICE pointers
 * (count elements of dtype / one double); the hook must sum them over all shards in
 * place and return 0.  The stream is idle when the hook runs. */
typedef int (*dca_reduce_hook)(void* user, void* g_dev, size_t count, int dtype, void* fx_dev);
int dca_plm_set_reduce_hook(dca_ctx* ctx, dca_reduce_hook hook, void* user);

/* Sharded optimiser state (optional, on top of sequence sharding).  With a comm hook set the
 * P-vectors of the L-BFGS (x_prev, g, g_prev, d, 5 x (s, y)) are only maintained on this rank's
 * slice: an evaluation ends with REDUCE_SCATTER of the local gradients (instead of the all-reduce of
 * dca_plm_set_reduce_hook, which is then not used), a step ends with ALL_GATHER of x, and the dot
 * products are ALL_REDUCEd as a handful of doubles.  Same bytes on the wire as one all-reduce per
 * evaluation, but the vector work is divided by `world`.  The hook works on DEVICE memory, in place:
 *   DCA_COMM_ALL_REDUCE     buf[0..count) summed over the ranks (dtype DCA_F64 scalars)
 *   DCA_COMM_REDUCE_SCATTER buf[0..count) summed; the rank needs only its slice afterwards
 *   DCA_COMM_ALL_GATHER     the rank's slice of buf is valid; all of buf[0..count) afterwards
 * count is a multiple of world; rank r's slice is [r * count / world, (r + 1) * count / world).
 * The context's stream is idle when the hook runs.  Call after dca_plm_configure. */
enum { DCA_COMM_ALL_REDUCE = 0, DCA_COMM_REDUCE_SCATTER = 1, DCA_COMM_ALL_GATHER = 2 };
typedef int (*dca_comm_hook)(void* user, int op, void* buf_dev, size_t count, int dtype);
int dca_plm_set_vector_sharding(dca_ctx* ctx, int rank, int world, dca_comm_hook hook, void* user);

typedef struct {
    int status;        /* libLBFGS code as the reference would report it (lbfgs.h:76-149): 0, -997, -998, -1001 ... */
    int iterations;    /* completed iterations since dca_plm_lbfgs_begin */
    int evaluations;   /* objective/gradient evaluations since dca_plm_lbfgs_begin */
    int finished;      /* 1 once a terminal status was reached */
    double fx, xnorm, gnorm, step;
    double seconds;    /* wall time spent inside dca_plm_lbfgs_iterate so far */
} dca_plm_stats;

/* L-BFGS with More-Thuente line search and the backend's parameters
 * (plmdcaBackend.cpp:68-75: m=5, epsilon=1e-3, max_linesearch=5, ftol=1e-4; the rest
 * libLBFGS defaults, lbfgs.cpp:116-121).  begin() evaluates at the current x;
 * iterate() runs up to `iterations` more iterations (resumable); max_iterations is the
 * reference's cap (-997 when exceeded; 0 = unlimited). */
int dca_plm_lbfgs_begin(dca_ctx* ctx, int max_iterations, int verbose);
int dca_plm_lbfgs_iterate(dca_ctx* ctx, int iterations, dca_plm_stats* stats_out);
/* Abandons the optimisation in progress (x and g keep their current values): the exchange scheme, the decomposition and the
 * communicator may change again.  A run that reached its cap or converged has ended by itself.  No reference counterpart
 * (lbfgs() runs to completion, lbfgs.cpp:248-644); needed because dca_plm_lbfgs_iterate is resumable. */
int dca_plm_lbfgs_end(dca_ctx* ctx);

/* ------------------------------------------------------------------ one call
 * The reference's single entry plmdcaBackend(biomolecule, num_site_states, msa_file, seqs_len, seqid, lambda_h, lambda_J,
 * max_iteration, num_threads, verbose) (plmdcaBackend.cpp:151-201) with a device list in place of num_threads, either a file (one
 * sequence per line, the reference's reader and its first-occurrence dedup) or a pre-encoded alignment, and what the reference
 * drops -- status, iterations, evaluations, fx, norms, seconds -- in dca_plm_stats.  Several devices: one rank per device as one
 * host thread each (no helper process), column-strip decomposition over the library's RCCL communicators; float64 gives the
 * single-device bytes.  x_out: P = L q + L (L - 1) / 2 q^2 elements of x_dtype (DCA_F32 | DCA_F64), packed as
 * plmdca_numerics.cpp:467-480.  Errors as everywhere: DCA_ERR_* and dca_last_error(). */
typedef struct dca_plm_args {
    int biomolecule;             /* DCA_BIOMOLECULE_PROTEIN (q = 21) | DCA_BIOMOLECULE_RNA (q = 5) */
    const char* msa_file;        /* one sequence per line (as plmdcaBackend reads it), or NULL */
    const uint8_t* msa;          /* ... or num_seqs x seqs_len codes < q, gap = q - 1 (as dca_set_msa takes them) */
    int num_seqs, seqs_len;      /* seqs_len is needed with a file as well (as plmdcaBackend's seqs_len) */
    float seqid, lambda_h, lambda_J;
    int max_iterations;          /* the reference's cap (0: unlimited) */
    int precision;               /* DCA_F32: the reference's arithmetic; DCA_F64: the parity mode */
    const int* devices;          /* GPU indices, one rank each; NULL / num_devices 0: device 0 */
    int num_devices;
    int exchange_scheme;         /* 0 (default) or 4: column strips */
    const char* rccl_path;       /* NULL: the librccl next to the HIP runtime in use (DCA_RCCL_PATH overrides) */
    int verbose;                 /* the reference's per-iteration lines on stderr (rank 0) */
} dca_plm_args;
int dca_plm_run(const dca_plm_args* args, void* x_out, int x_dtype, dca_plm_stats* stats_out);

/* Frobenius-norm scores of the current x: PlmDCA.get_couplings_no_gap_state +
 * compute_sorted_FN / compute_sorted_FN_APC (plmdca.py:246-268, :437-524), in pair
 * order (0,1),(0,2)...; sorting is left to the host. */
int dca_plm_scores(dca_ctx* ctx, int apc, double* scores_out);

/* Direct-information scores of the current x (PlmDCA.compute_direct_info_unsorted_DI /
 * compute_sorted_DI[_APC], plmdca.py:683-790, numerics plmdca/msa_numerics.py:156-311) in pair
 * order.  reg_fi: L*q regularised single-site frequencies (the reference computes them from
 * its Python reader's alignment with pseudocount 0.5, plmdca.py:622-648). */
int dca_plm_di_scores(dca_ctx* ctx, const double* reg_fi, int apc, double* scores_out);

/* (q-1)x(q-1) coupling blocks of the current x for `npairs` site pairs (pairs[2k] < pairs[2k+1]),
 * row-major a,b, as doubles; shift != 0 applies the zero-sum gauge of PlmDCA.shift_couplings
 * (plmdca.py:320-342).  Feeds PlmDCA.compute_params (plmdca.py:345-434). */
int dca_plm_pair_couplings(dca_ctx* ctx, const int* pairs, int npairs, int shift, double* out);

/* Statistical energies of n query sequences X (n x L codes < q, gap = q-1; host) under the current x:
 *   E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j)
 * with h and J the parameter vector exactly as stored (fields L*q first, then the q x q blocks in pair order; gap state
 * included; float32 values in the float32 mode, float64 in the float64 mode).  Higher is more probable.  Every term is
 * widened to double and summed in double in an order fixed by (L, q, precision) alone: a sequence's energy is bitwise the
 * same whatever n, its position among the queries, or the call.  The query rows go to a buffer of their own; the context's
 * alignment, weights and optimiser state are not touched.  n == 0 is DCA_OK; a code >= q is DCA_ERR_ARG; DCA_ERR_STATE before
 * dca_plm_configure.  Column strips: collective, like dca_plm_scores.  No reference counterpart (pydca only ranks pairs). */
int dca_plm_energies(dca_ctx* ctx, const uint8_t* X, int n, double* energies_out);
/* Single-mutant effects of the wild type w (L codes): dE[i*q + a] = E(w with w_i -> a) - E(w)
 *   = h_i(a) - h_i(w_i) + sum_{j != i} [J_ij(a, w_j) - J_ij(w_i, w_j)]
 * for every site i and every state a (gap included), summed in double over ascending j; dE[i*q + w_i] = 0.0 exactly. */
int dca_plm_mutation_scan(dca_ctx* ctx, const uint8_t* wildtype, double* dE_out /* L*q */);
/* Site conditionals and pseudo-log-likelihoods of n query sequences X (n x L codes < q, gap = q-1; host) under the current x
 * (h and J exactly as dca_plm_energies defines them, gap state included):
 *   u_i(a) = h_i(a) + sum_{j != i} J_ij(a, s_j)      (J_ij for i > j is J_ji transposed)
 *   m_i = max_b u_i(b),  Z_i = sum_b exp(u_i(b) - m_i) (ascending b),  cond[i][a] = (u_i(a) - m_i) - log Z_i = log P(s_i = a | s_-i)
 *   site[i] = cond[i][s_i],  PLL(s) = sum_i site[i] (ascending i).
 * Every term is widened to double and summed in double without contraction: h_i(a) first, then j ascending; the order depends
 * on (L, q, precision) alone.  A sequence's outputs have the same bits whatever n, its position among the queries, the passes
 * the call splits the queries into, or the call.  Outputs (host): pll_out[n]; site_out[n*L] (row n, site i at n*L + i) and
 * cond_out[n*L*q] (at (n*L + i)*q + a) when not NULL.  The alignment, the weights, x, g and the optimiser state are not
 * touched; an L-BFGS or Boltzmann-learning run in progress is allowed.  n == 0 is DCA_OK; a code >= q is DCA_ERR_ARG;
 * DCA_ERR_STATE before dca_plm_configure.  Column strips: collective, like dca_plm_energies.  This is the true PLL: with
 * carry_mode CARRY_EXACT and no regulariser, the fx of dca_plm_gradient is -sum_n w_n PLL(s_n) over the context's alignment;
 * the other carry modes differ from it by design.  Profiling tag "pll".  No reference counterpart. */
int dca_plm_pseudo_likelihood(dca_ctx* ctx, const uint8_t* X, int n, double* pll_out /* n */, double* site_out /* n*L or NULL */,
                              double* cond_out /* n*L*q or NULL */);
/* Systematic-scan Gibbs sampling of n independent chains from P(s) ~ exp(beta * E(s)) under the current x (E as in
 * dca_plm_energies).  One sweep visits sites i = 0 .. L-1 in order; at site i a chain forms u_i(a) = h_i(a) + sum_{j != i} J(a, s_j)
 * for every state a < q (gap included; every term in double, in an order fixed by (L, q, precision)), sets
 * p_a = exp(beta * (u_i(a) - max_b u_i(b))), T = sum_a p_a (ascending a), r = U * T, and takes the smallest a whose ascending
 * cumulative sum exceeds r (the largest a with p_a > 0 if rounding leaves none).  U is the uniform of Philox4x32-10 with
 * key (seed & 0xffffffff, seed >> 32) and counter (chain, sweep, site, 0), chain = first_chain + k, sweep = first_sweep + t
 * (each word mod 2^32): U = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53.  initial: n x L codes < q (host), or NULL: chain k starts
 * from s_i = floor(U * q) with counter (chain, 0, i, 1).  out: n x L codes (host) after `sweeps` sweeps (sweeps = 0 returns the
 * start).  Chain k's result depends only on the model, seed, first_chain + k, first_sweep, sweeps, its start and beta: the same
 * bits in any batch or split of one, and a + b sweeps equal a sweeps continued with first_sweep = a from their output.
 * One launch per sweep on the context's stream.  The alignment, weights, x, g and the optimiser are not touched.
 * DCA_ERR_ARG: n < 0, sweeps < 0, beta < 0, NaN or infinite, an initial code >= q, out NULL with n > 0; n == 0 is DCA_OK;
 * DCA_ERR_STATE before dca_plm_configure.  Column strips: collective, like dca_plm_energies.  No reference counterpart. */
int dca_plm_sample(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                   const uint8_t* initial, uint8_t* out);
/* Conditional Gibbs sampling: dca_plm_sample with every site outside free_sites clamped.  free_sites:
 * num_free = F distinct site indices in [0, L), strictly ascending, f_0 < ... < f_{F-1}; chain k keeps initial[k][j] at every
 * other site j for ever.  initial (n x L codes < q, host) is required: each chain carries its own background.  random_start != 0:
 * free site i of chain c starts from floor(U * q) with the Philox counter (chain, 0, i, 1), dca_plm_sample's start at that site;
 * random_start == 0: the free sites start from initial.
 * The sweep with global number first_sweep + t visits the free sites in ascending order.  At free site i = f_kappa a chain forms,
 * every term widened to double and no contraction,
 *   c_i(a) = h_i(a) + sum over the clamped j, ascending, of J_ij(a, s_j)    (once per call; h first, then j ascending, one
 *                                                                           sequential double sum)
 *   u_i(a) = (((c_i(a) + S_0(a)) + S_1(a)) + S_2(a)) + S_3(a),  S_w(a) = sum over the free positions k = w (mod 4), k != kappa,
 *            ascending k, of J(a, s_{f_k})    (the terms of S_0 join c_i(a) one by one, as in dca_plm_sample; S_1 .. S_3 start from 0)
 * and draws by dca_plm_sample's rule: p_a = exp(beta * (u(a) - max_b u(b))), T the ascending sum, r = U * T, the smallest a whose
 * cumulative sum exceeds r (the largest a with p_a > 0 if rounding leaves none), U from the Philox counter (chain, sweep, i, 0):
 * the site word is the site index i, not the position kappa.  So with F = L the entry is bit for bit dca_plm_sample; chain k's
 * result depends only on the model, seed, first_chain + k, first_sweep, sweeps, its row of initial, the site list, random_start
 * and beta (the same bits in any batch, split or pass); and a + b sweeps equal a sweeps continued with first_sweep = a and
 * random_start = 0.  out: n x L codes (host); F == 0 or sweeps == 0 returns the start state.
 * A sweep reads only the F x F sub-table of the couplings; the field buffer (n x F x q doubles) is bounded at 1 GiB by running
 * blocks of chains (multiples of 64; DCA_COND_PASS caps the block) one after another.
 * DCA_ERR_ARG: n < 0, sweeps < 0, beta < 0, NaN or infinite, initial or out NULL with n > 0, num_free outside [0, L], free_sites
 * NULL with num_free > 0, an index out of range or not strictly ascending, an initial code >= q; n == 0 is DCA_OK.
 * DCA_ERR_STATE: before dca_plm_configure; under column strips, vector sharding, a reduce / comm hook or a native-comm mode (one
 * GPU only, like dca_plm_ais).  An L-BFGS or Boltzmann-learning run in progress is allowed; the alignment, the weights, x, g, the
 * optimiser and the bmDCA chains are not touched.  Profiling tags: "cond_fields" (one pass per block of chains), "sample_cond"
 * (one launch per sweep and block).  No reference counterpart. */
int dca_plm_sample_conditional(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep,
                               double beta, const int32_t* free_sites, int num_free, const uint8_t* initial /* n x L, required */,
                               int random_start, uint8_t* out /* n x L */);

/* Greedy ascent to a local maximum of E (as dca_plm_energies defines it, gap state included) over a list of free sites, every other
 * site clamped to the chain's own row of X.  free_sites: as in dca_plm_sample_conditional (num_free = F
 * strictly ascending indices in [0, L)); NULL with 0 does NOT mean "all sites": pass 0 .. L-1.  Chain k, started at row k of X, does,
 * every value widened to double and no contraction:
 *   1. table: for every free site i and state a, U_i(a) = h_i(a) + sum over j != i, ascending j, of J_ij(a, s_j): one sequential
 *      double sum, h first, then j ascending (the order of dca_plm_pseudo_likelihood's u_i(a)).  Clamped sites contribute here and
 *      never again.
 *   2. step t: g(i, a) = U_i(a) - U_i(s_i) for free i and a != s_i; the largest g wins, ties go to the smallest i, then the
 *      smallest a.  If g > min_gain and t < max_steps the move is applied, otherwise the chain stops.
 *   3. apply (i*, a*), old = s_i*: s_i* <- a*, and for every free j != i* and every b, U_j(b) <- U_j(b) + (J_{j i*}(b, a*) -
 *      J_{j i*}(b, old)), the difference formed first, in double.  U_i* is unchanged.
 * out: the final codes (n x L; clamped columns are those of X).  steps_out: the number of applied steps.  converged_out: 1 if the
 * chain stopped because no g exceeded min_gain (also when that happens at t == max_steps, and with F == 0), 0 if it stopped at
 * max_steps with a g > min_gain left.  gain_out (or NULL): the sequential double sum of the applied g.  path_out (or NULL; n x
 * max_steps x 2: site, new state) and path_gain_out (or NULL; n x max_steps): one record per applied step, -1 / -1 / 0.0 past
 * steps_out.  With max_steps = 0 or F = 0, out = X.
 * A chain's result depends only on the model, its row of X, the site list, max_steps and min_gain: the same bits in any batch,
 * split or pass, and wherever the table is kept.  Continuing an unconverged chain from its output forms the table afresh, so the
 * continuation equals the uninterrupted run wherever the incrementally updated table has not drifted from a fresh one (it cannot
 * when every partial sum is exact); nothing more is promised.
 * The table (F x q doubles per chain) sits in LDS when it and the site list and codes fit (DCA_ASCENT_LDS: the largest table in
 * bytes that may; 0 keeps it in device memory), and the device scratch is bounded at 1 GiB by running blocks of chains
 * (DCA_ASCENT_PASS caps the block) one after another.
 * DCA_ERR_ARG: n < 0, max_steps < 0, min_gain negative, NaN or infinite, X, out, steps_out or converged_out NULL with n > 0,
 * num_free outside [0, L], free_sites NULL with num_free > 0, an index out of range or not strictly ascending, a code of X >= q;
 * n == 0 is DCA_OK.  DCA_ERR_STATE: before dca_plm_configure; under column strips, vector sharding, a reduce / comm hook or a
 * native-comm mode (one GPU only, like dca_plm_sample_conditional).  An L-BFGS or Boltzmann-learning run in progress is allowed; the
 * alignment, the weights, x, g, the optimiser and the bmDCA chains are not touched.  Profiling tags: "ascent_init" (the table, one
 * pass per block of chains), "ascent" (one launch per block: all steps of all its chains).  No reference counterpart. */
int dca_plm_ascend(dca_ctx* ctx, const uint8_t* X /* n x L */, int n, const int32_t* free_sites, int num_free, int max_steps,
                   double min_gain, uint8_t* out /* n x L */, int32_t* steps_out /* n */, uint8_t* converged_out /* n */,
                   double* gain_out /* n, or NULL */, int32_t* path_out /* n x max_steps x 2, or NULL */,
                   double* path_gain_out /* n x max_steps, or NULL */);

/* Replica-exchange (parallel-tempering) Gibbs sampling on a temperature ladder: M ladders of R walkers,
 * n = M R walkers in all, betas[0] < ... < betas[R-1].  Walker r of ladder m is row m R + r of every per-walker array; its Philox
 * chain word is (first_ladder + m) R + r.  It starts at level r, or at initial_levels[m R + r] (within each ladder a permutation
 * of 0 .. R-1), from the tag-1 random state of its chain word (dca_plm_sample's start), or from row m R + r of initial.  A walker
 * keeps its codes for ever; what the exchanges move is its level.
 * The sweep with global number g = first_sweep + t is dca_plm_sample's sweep (same summation order, draw rule and Philox counter
 * (chain, g, site, 0)) with every walker under betas[level(walker)]: p_a = exp(beta_c * (u(a) - max_b u(b))).
 * Exchange rounds: after global sweep g, if swap_interval = I > 0 and (g + 1) mod I == 0, round rho = (g + 1) / I - 1 runs.  E of
 * every walker is formed bit for bit as dca_plm_energies forms it for the walker's codes.  For each ladder and each k with
 * k = rho (mod 2) and k + 1 < R, with a the walker at level k and b the walker at level k + 1:
 *   d = (betas[k+1] - betas[k]) * (E_a - E_b)    (both differences first, then one multiply, in double, no contraction)
 *   U = the Philox uniform of key (seed) and counter (first_ladder + m, rho, k, 5)    (tag 5; U as in dca_plm_sample)
 *   accept iff d >= 0 || U < exp(d);  accepting exchanges the levels of a and b (and so their beta); codes never move.
 * The pairs of a round are disjoint.  rounds = floor((first_sweep + sweeps) / I) - floor(first_sweep / I) (0 when I == 0).
 * Outputs (host): out, the codes after `sweeps` sweeps; levels_out, each walker's level then; energies_out (or NULL), E of the
 * final codes (bit for bit dca_plm_energies of out); attempts_out / accepts_out (or NULL; R-1 each), the exchanges attempted and
 * accepted between levels k and k + 1, summed over ladders and rounds; energy_trace_out (or NULL; rounds x M x R),
 * trace[round][m][k] = E of the walker at level k before that round's exchange, rounds counted from the call's first;
 * rounds_out (or NULL).
 * Guarantees:
 *   (a) with swap_interval == 0, row m R + r is bit for bit dca_plm_sample(1, sweeps, seed, (first_ladder + m) R + r, first_sweep,
 *       betas[r], its start);
 *   (b) a ladder's outputs depend only on the model, seed, first_ladder + m, betas, first_sweep, sweeps, I and its starts: the
 *       same bits in any batch or split by ladders (the counters are sums over the ladders);
 *   (c) a + b sweeps equal a sweeps continued from out / levels_out with first_sweep = a, for any a: rounds are numbered
 *       globally (the counters and trace rows of the two parts add up to the whole run's).
 * One launch per sweep for all walkers; nothing goes to the host between rounds except the trace.  The device scratch (state,
 * energies' slabs, trace buffer) stays within 1 GiB: blocks of ladders run one after another (DCA_PT_PASS caps the ladders of a
 * block) and the trace buffer (at most 256 MiB) is flushed in blocks of rounds (DCA_PT_TRACE_ROUNDS caps them); neither shows
 * in the results.
 * DCA_ERR_ARG: args NULL, ladders < 0, levels < 1, sweeps < 0, swap_interval < 0, more than 2^24 walkers, first_sweep + sweeps
 * past 2^64 - 1, betas NULL, a beta that is negative, NaN, infinite or not above its predecessor, out or levels_out NULL with
 * M > 0, initial_levels that are not a permutation within a ladder, an initial code >= q; M == 0 is DCA_OK.
 * DCA_ERR_STATE: before dca_plm_configure; under column strips, vector sharding, a reduce / comm hook or a native-comm mode (one
 * GPU only, like dca_plm_sample_conditional).  An L-BFGS or Boltzmann-learning run in progress is allowed; the alignment, the
 * weights, x, g, the optimiser and the bmDCA chains are not touched.  Profiling tags: "sample" (the sweeps), "pt_energy" (the
 * energy pass of a round), "pt_swap" (the exchange kernel).  No reference counterpart. */
typedef struct dca_pt_args {
    int ladders, levels;             /* M >= 0, R >= 1 */
    const double* betas;             /* R values: finite, >= 0, strictly increasing */
    int sweeps, swap_interval;       /* >= 0; swap_interval 0: no exchange */
    uint64_t seed, first_ladder, first_sweep;
    const uint8_t* initial;          /* M*R x L codes < q, or NULL */
    const int32_t* initial_levels;   /* M*R, or NULL: walker r at level r */
} dca_pt_args;
int dca_plm_sample_tempered(dca_ctx* ctx, const dca_pt_args* args, uint8_t* out /* M*R x L */, int32_t* levels_out /* M*R */,
                            double* energies_out /* M*R or NULL: E of the final codes */, uint64_t* attempts_out,
                            uint64_t* accepts_out /* R-1 each, or NULL */, double* energy_trace_out /* rounds x M x R, or NULL */,
                            int* rounds_out /* or NULL */);

/* ------------------------------------------------------------------ Boltzmann machine learning (bmDCA) of the plm model
 * Refines the context's x (fields h: L*q, then the q x q blocks J_ij, i < j, pair order; storage precision P = the context's
 * float32 / float64) by gradient ascent on the L2-regularised log-likelihood per effective sequence, with the model's
 * frequencies estimated from n persistent Gibbs chains kept on the device.  q states, gap (q-1) included everywhere.
 *
 * Data statistics, formed once by dca_plm_bm_begin from the alignment X (N x L) and its current weights w: Meff = sum_n w_n,
 * f_i(a) = sum_n w_n [X_ni = a] / Meff, f_ij(a,b) likewise (i < j), then f^_i = (1 - lambda) f_i + lambda / q and
 * f^_ij = (1 - lambda) f_ij + lambda / q^2 (lambda = pseudocount); every operation rounded in double in the order written.
 * With integer weights every count is exact.
 *
 * Chains and sweeps: chain k is Philox chain k and follows dca_plm_sample's draw rule with beta = 1; it starts at the tag-1 random
 * state or at row k of `initial`.  Sweeps 0 .. E-1 (equilibration) run under the starting x.  Iteration t (counted from begin
 * across iterate calls) runs sweeps E + t k .. E + t k + k - 1 under the current x.  So with eta_h = eta_J = 0 the chains after
 * T iterations are bit for bit dca_plm_sample(n, E + T k, seed, 0, 0, 1.0, initial), and x does not change.
 *
 * Model statistics after iteration t's sweeps: integer counts c_i(a), c_ij(a,b) over the n chains, g_i = c_i / n,
 * g_ij = c_ij / n (one correctly rounded division each).
 * Update of every parameter theta with its f^, g, rate eta (eta_h fields, eta_J couplings) and L2 weight mu (mu_h, mu_J):
 * d = f^ - g, r = mu * theta, s = d - r, theta' = theta + eta * s, in double with theta widened, rounded once to P.
 *
 * Record of iteration t (the chains after its sweeps, before its update: it describes the x the sweeps ran under):
 * eps_h = max |f^_i(a) - g_i(a)|, eps_J = max over i < j, a, b of |f^_ij - g_ij|, pearson = the Pearson correlation over the
 * M = pairs * q^2 values of C^d = f^_ij - f^_i f^_j and C^m = g_ij - g_i g_j:  with the sums S_d, S_m, S_dd, S_mm, S_dm,
 * cov = S_dm / M - (S_d / M)(S_m / M), v_d = S_dd / M - (S_d / M)^2, v_m likewise, pearson = cov / sqrt(v_d v_m) (0 when
 * v_d v_m <= 0).  The sums run in double in an order fixed by (L, q): repeated runs give the same bits.
 *
 * State: DCA_ERR_STATE before dca_plm_configure, during an L-BFGS run (dca_plm_lbfgs_end first), under column strips, vector
 * sharding, a reduce / comm hook or a native-comm mode (one GPU only); iterate / freqs / chains without a run.  A run ends with
 * dca_set_msa, any weights call, dca_plm_configure(_strips), dca_plm_lbfgs_begin, dca_plm_release and dca_plm_bm_end;
 * dca_plm_bm_begin during a run starts a new one.  dca_plm_set_x during a run is allowed: the next iteration continues from it.
 * The run never touches the alignment, the weights or g; x is the context's x, so energies, scans, sampling and scores read the
 * refined model.  Profiling tags: the sweeps "sample", the statistics and update launches "bm_stats".  No reference counterpart. */
typedef struct dca_bm_args {
    int chains, sweeps, equilibration_sweeps;   /* n >= 1, k >= 1, E >= 0 */
    uint64_t seed;
    double eta_h, eta_J, mu_h, mu_J;            /* >= 0, finite */
    double pseudocount;                         /* [0, 1) */
    const uint8_t* initial;                     /* n x L host codes < q, or NULL: random starts */
} dca_bm_args;
typedef struct { double eps_h, eps_J, pearson; } dca_bm_record;
/* data statistics, chains, E sweeps.  DCA_ERR_ARG: args NULL or out of range, an initial code >= q */
int dca_plm_bm_begin(dca_ctx* ctx, const dca_bm_args* args);
/* `iterations` iterations (0: nothing; < 0: DCA_ERR_ARG); records_out: iterations records, or NULL */
int dca_plm_bm_iterate(dca_ctx* ctx, int iterations, dca_bm_record* records_out);
/* which 0: f^ (the data); 1: g of the last iteration (DCA_ERR_STATE before the first); either output may be NULL.
 * fi_out: L*q, fij_out: pairs*q*q in pair order.  DCA_ERR_ARG for another `which` */
int dca_plm_bm_freqs(dca_ctx* ctx, int which, double* fi_out, double* fij_out);
/* the chains' current codes, n x L (DCA_ERR_ARG: out NULL) */
int dca_plm_bm_chains(dca_ctx* ctx, uint8_t* out);
/* ends the run (x keeps its refined values); DCA_OK without a run */
int dca_plm_bm_end(dca_ctx* ctx);

/* ------------------------------------------------------------------ sparse bmDCA: a mask on the couplings and their decimation
 * (Barrat-Charlaix, Muntoni, Weigt 2021).  A run may carry a mask of pairs*q*q bytes in pair order, 1 =
 * active; a run starts without one (all active), and a mask ends with its run (dca_plm_bm_end, a new dca_plm_bm_begin, and
 * everything else that ends a run).  With a mask, the update of an iteration writes exactly +0 to a removed coupling element and
 * updates the active ones as always; fields are never masked; the record stays defined over all pairs*q^2 elements.  A mask of
 * all ones gives the bits of a run without one.  dca_plm_set_x during a masked run is allowed and leaves x as given: the next
 * iteration's update zeroes the removed elements again.
 *
 * dca_plm_bm_set_mask installs a mask and writes +0 to x at its zeros.  DCA_ERR_ARG: mask NULL or a value above 1; DCA_ERR_STATE
 * without a run.  dca_plm_bm_get_mask: the mask, all ones if none was installed (DCA_ERR_ARG: out NULL; DCA_ERR_STATE
 * without a run).
 *
 * dca_plm_bm_decimate scores every active element and removes the `remove` lowest.
 * Frequencies: p = c_ij(a,b) / n of the chains as they are (the integer counts behind dca_plm_bm_freqs(ctx, 1, ..), one division).
 * Score: D = the symmetrised Kullback-Leibler divergence between the model and the model with this element set to zero,
 * J (p - p'), p' = p e^-J / (1 - p + p e^-J), computed in double, J the element widened, in this operation order:
 *   p == 0 or p == 1 or J == 0:  D = +0
 *   J > 0:  e = expm1(-J),  D = ((J * (-e)) * (p * (1 - p))) / (1 + p * e)
 *   J < 0:  e = expm1(J),   D = ((J * e) * (p * (1 - p))) / (1 + (1 - p) * e)
 * and -0 made +0; D >= +0.  A removed element's score is -1.0 and it takes no part in the selection.
 * Selection: the `remove` active elements smallest under (D's bit pattern as an unsigned 64-bit integer, then the element's offset
 * in pair order); exact, and the same for every launch geometry.  They get x = +0 and mask = 0 (the mask is created if absent;
 * remove == 0 touches neither x nor the mask).  scores_out: the scores the selection ran on.  info: active_before, removed,
 * active_after, threshold = the largest removed D, removed_sum = the sum of the removed D added one by one in ascending key
 * order (both +0 when nothing was removed).
 * DCA_ERR_STATE without a run or before the first iteration; DCA_ERR_ARG for remove < 0 or remove > the active elements.
 * Profiling tag "bm_decimate". */
typedef struct { long long active_before, removed, active_after; double threshold, removed_sum; } dca_bm_decimation;
int dca_plm_bm_set_mask(dca_ctx* ctx, const uint8_t* mask /* pairs*q*q, 0/1 */);
int dca_plm_bm_get_mask(dca_ctx* ctx, uint8_t* out /* pairs*q*q */);
int dca_plm_bm_decimate(dca_ctx* ctx, long long remove, double* scores_out /* pairs*q*q or NULL */, dca_bm_decimation* info /* or NULL */);

/* Moves the context's x (fields L*q, then the q x q blocks in pair order) to the zero-sum gauge in place: every block's rows and
 * columns sum to zero, every site's fields sum to zero, and the energy of every sequence changes by one common constant, which
 * is not kept.  Every operation in double in this order, rounded once to the storage precision:
 *   per pair i < j:  r(a) = (sum_b J(a,b)) / q,  c(b) = (sum_a J(a,b)) / q,  m = (sum_a r(a)) / q, each sum from 0.0 in ascending
 *                    index;  J'(a,b) = ((J(a,b) - r(a)) - c(b)) + m;  the block hands r(a) - m to site i and c(b) - m to site j;
 *   per site i:      t(a) = h_i(a), then for j = 0 .. L-1 (j != i) in ascending order t(a) += the part pair (i,j) hands to i;
 *                    u = (sum_a t(a)) / q from 0.0 in ascending a;  h'_i(a) = t(a) - u.
 * State: as dca_plm_set_x (after dca_plm_configure; an L-BFGS or Boltzmann run in progress continues from the new x), on one GPU
 * only (DCA_ERR_STATE under column strips, vector sharding, a reduce / comm hook or a native-comm mode), and DCA_ERR_STATE
 * during a Boltzmann run whose mask has removed elements: the transformation would fill them again.  Profiling tag "gauge". */
int dca_plm_zero_sum_gauge(dca_ctx* ctx);

/* ------------------------------------------------------------------ log Z by annealed importance sampling (AIS; Neal 2001)
 * Estimates Z = sum_s exp(E(s)) of the current x (E exactly as dca_plm_energies defines it, gap state included).
 * h0: base fields, L*q finite host doubles, or NULL: the model's own fields h.  E0(s) = sum_i h0_i(s_i), in double over
 * ascending i; dE = E - E0; the path is E_beta = E0 + beta * dE with 0 = beta_0 < beta_1 < ... < beta_K = 1 (K >= 1; betas NULL:
 * beta_k = k / K in double).
 * Start: chain c (= first_chain + c) draws x_0 exactly from p0(s) ~ exp(E0(s)): at site i, p_a = exp(h0_i(a) - max_b h0_i(b)) and
 *   the samplers' draw rule with the Philox counter (chain, 0, i, 2) (tag 2; tags 0 and 1 keep their meaning).
 * Transitions: for k = 1 .. K-1, s Gibbs sweeps under E_{beta_k}, numbered and drawn exactly as dca_plm_sample (tag 0, global sweep
 *   numbers (k-1)s .. ks-1, ascending sites) except that the conditional is c_i(a) = h0_i(a) + beta_k * (u_i(a) - h0_i(a)), u_i(a)
 *   the sampler's double sum (same order), and p_a = exp(c_i(a) - max_b c_i(b)).  No sweep runs at beta_K = 1.
 * Weights: log w = 0.0; for k = 1 .. K: log w <- log w + (beta_k - beta_{k-1}) * (E(x_{k-1}) - E0(x_{k-1})), every operation rounded in
 *   double in the order written (no fused multiply-add); E(x) here is bit for bit what dca_plm_energies returns for those codes.
 * Outputs: log_weights_out (n), log_z0_out = log sum_s exp(E0(s)) as dca_ais_estimate wants it (may be NULL), chains_out: the n x L
 *   codes x_{K-1} after the last transition (may be NULL).  Chain c's codes and log w depend only on the model, h0, the schedule, s,
 *   the seed and first_chain + c: the same bits in any batch or split.
 * DCA_ERR_ARG: args or log_weights_out NULL, n < 1 or n > 2^24, K < 1, s < 0, betas not finite, not strictly increasing or not from
 *   0 to 1, a base field not finite.  DCA_ERR_STATE before dca_plm_configure, under column strips, vector sharding, a reduce / comm
 *   hook or a native-comm mode (one GPU only); an L-BFGS run in progress is allowed, as for dca_plm_sample.
 * The call touches neither the alignment, the weights, x, g, the optimiser nor a bmDCA run in progress (its chains and its next
 * iteration keep their bits).  Nothing leaves the device between temperatures.  Profiling tags: the sweeps "sample", the start draw
 * and the weight updates "ais".  No reference counterpart. */
typedef struct dca_ais_args {
    int chains;                   /* n >= 1 */
    int temperatures;             /* K >= 1 */
    const double* betas;          /* K + 1 values as above, or NULL: k / K */
    int sweeps_per_temperature;   /* s >= 0 */
    uint64_t seed, first_chain;
    const double* base_fields;    /* L*q host doubles, or NULL: the model's own fields */
} dca_ais_args;
int dca_plm_ais(dca_ctx* ctx, const dca_ais_args* args, double* log_weights_out /* n */, double* log_z0_out,
                uint8_t* chains_out /* n x L, or NULL */);
/* The estimate from n log weights, on the host in a fixed order (needs no device):
 *   log Z0 = sum_i (m_i + log sum_a exp(h0_i(a) - m_i)), m_i = max_a h0_i(a) (what the AIS entries return);
 *   m = max_c log w_c, S1 = sum_c exp(log w_c - m), S2 = sum_c exp(2 (log w_c - m)), both over ascending c;
 *   log Z = ((log Z0 + m) + log S1) - log n;  ESS = S1 S1 / S2;  stderr(log Z) = sqrt(max(0, S2 / (S1 S1) - 1 / n)), the
 *   delta-method error of log-mean-w.  Outputs may be NULL.  DCA_ERR_ARG: log_weights NULL, n < 1, a value not finite. */
int dca_ais_estimate(const double* log_weights, int n, double log_z0, double* log_z, double* ess, double* stderr_log_z);

/* ------------------------------------------------------------------ DI on caller-provided arrays
 * The module-level functions of the reference: compute_two_site_model_fields + compute_direct_info
 * (meanfield_dca/msa_numerics.py:378-533: layout 1 = couplings as the n x n matrix, n = L(q-1);
 * plmdca/msa_numerics.py:156-311: layout 2 = gap-stripped blocks, pair order, (q-1)^2 each).
 * All arrays are HOST doubles; reg_fi is L x q; fields_out (optional) receives [pairs][2][q],
 * di_out (optional) [pairs].  No alignment needs to be set on the context. */
int dca_di_from_arrays(dca_ctx* ctx, const double* couplings, int layout, const double* reg_fi, int L, int q,
                       double* fields_out, double* di_out);

/* compute_direct_info with the caller's own two-site model fields (its `fields_ij` argument,
 * meanfield_dca/msa_numerics.py:473-533, plmdca/msa_numerics.py:249-311): fields_ij is [pairs][2][q] HOST doubles
 * and is used as given -- no fixed-point iteration runs.  di_out: [pairs]. */
int dca_di_from_fields(dca_ctx* ctx, const double* couplings, int layout, const double* reg_fi, const double* fields_ij,
                       int L, int q, double* di_out);

/* ------------------------------------------------------------------ ranking
 * Pair indices of the most recent score vector computed on this context (dca_plm_scores,
 * dca_plm_di_scores, dca_mf_scores, dca_mf_di_scores, dca_mf_run, dca_ar_epistatic_scores) in descending score order,
 * equal scores in ascending pair order: the sorted(..., reverse=True) step of
 * compute_sorted_FN / _APC / DI (meanfield_dca.py:941, plmdca.py:479), done on the device copy. */
int dca_scores_order(dca_ctx* ctx, int32_t* order_out, int capacity);

/* ------------------------------------------------------------------ mfDCA
 * Stage functions mirror pydca/meanfield_dca/msa_numerics.py; all float64. */
int dca_mf_single_site_freqs(dca_ctx* ctx, double* fi_out /* L*q, gap last (:53-89) */);
int dca_mf_pair_site_freqs(dca_ctx* ctx, double* fij_out /* pairs*(q-1)^2 (:182-229) */);
/* regularise (:92-125, :231-267) + build the L(q-1) x L(q-1) correlation matrix (:270-318) */
int dca_mf_corr_mat(dca_ctx* ctx, double pseudocount, double* corr_out /* may be NULL */);
/* couplings = -inv(C) (:321-342) by blocked Cholesky on f64 MFMA */
int dca_mf_couplings(dca_ctx* ctx, double* couplings_out /* may be NULL */);
/* FN / FN_APC of the couplings (meanfield_dca.py:902-988), pair order */
int dca_mf_scores(dca_ctx* ctx, int apc, double* scores_out);
/* DI / DI_APC of the couplings (meanfield_dca.py:793-899; msa_numerics.py:378-533), pair order;
 * needs dca_mf_corr_mat + dca_mf_couplings (or dca_mf_run) first */
int dca_mf_di_scores(dca_ctx* ctx, int apc, double* scores_out);
/* local fields of the global model, L*(q-1) doubles (MeanFieldDCA.compute_fields,
 * meanfield_dca.py:588-633); needs the couplings */
int dca_mf_fields(dca_ctx* ctx, double* fields_out);
/* dca_plm_energies / dca_plm_mutation_scan under the mean-field model: J_ij(a, b) = couplings[(i,a),(j,b)] (the -inv(C) of
 * dca_mf_couplings) and h_i(a) = the fields of dca_mf_fields for a, b < q-1; both are 0 when a or b is the gap state q-1 (the
 * gauge of the mean-field model).  Same formulas, order, determinism and argument checks; DCA_ERR_STATE before
 * dca_mf_couplings. */
int dca_mf_energies(dca_ctx* ctx, const uint8_t* X, int n, double* energies_out);
int dca_mf_mutation_scan(dca_ctx* ctx, const uint8_t* wildtype, double* dE_out /* L*q */);
/* dca_plm_pseudo_likelihood under the mean-field model (J, h as in dca_mf_energies; zero on the gap state).  Same formulas,
 * order, determinism and argument checks; DCA_ERR_STATE before dca_mf_couplings. */
int dca_mf_pseudo_likelihood(dca_ctx* ctx, const uint8_t* X, int n, double* pll_out /* n */, double* site_out /* n*L or NULL */,
                             double* cond_out /* n*L*q or NULL */);
/* dca_plm_sample under the mean-field model (J, h as in dca_mf_energies; zero on the gap state).  Same rule, RNG layout,
 * determinism and argument checks; DCA_ERR_STATE before dca_mf_couplings. */
int dca_mf_sample(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep, double beta,
                  const uint8_t* initial, uint8_t* out);
/* dca_plm_ais under the mean-field model (E, h as in dca_mf_energies; base_fields NULL: those fields, 0 on the gap state).  Same
 * rules, RNG layout, determinism and argument checks; DCA_ERR_STATE before dca_mf_couplings. */
int dca_mf_ais(dca_ctx* ctx, const dca_ais_args* args, double* log_weights_out, double* log_z0_out, uint8_t* chains_out);
/* dca_plm_sample_conditional under the mean-field model (J, h as in dca_mf_energies; zero on the gap state; DESIGN.md section
 * 23).  Same rule, RNG layout, determinism and argument checks; with F = L bit for bit dca_mf_sample; DCA_ERR_STATE before
 * dca_mf_couplings. */
int dca_mf_sample_conditional(dca_ctx* ctx, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep,
                              double beta, const int32_t* free_sites, int num_free, const uint8_t* initial /* n x L, required */,
                              int random_start, uint8_t* out /* n x L */);
/* dca_plm_ascend under the mean-field model (J, h as in dca_mf_energies; zero on the gap state).  Same
 * rule, determinism and argument checks; DCA_ERR_STATE before dca_mf_couplings. */
int dca_mf_ascend(dca_ctx* ctx, const uint8_t* X /* n x L */, int n, const int32_t* free_sites, int num_free, int max_steps,
                  double min_gain, uint8_t* out /* n x L */, int32_t* steps_out /* n */, uint8_t* converged_out /* n */,
                  double* gain_out /* n, or NULL */, int32_t* path_out /* n x max_steps x 2, or NULL */,
                  double* path_gain_out /* n x max_steps, or NULL */);
/* dca_plm_sample_tempered under the mean-field model (J, h as in dca_mf_energies; zero on the gap state).
 * Same rule, RNG layout, guarantees (with dca_mf_sample and dca_mf_energies in the place of the plm entries) and argument
 * checks; DCA_ERR_STATE before dca_mf_couplings. */
int dca_mf_sample_tempered(dca_ctx* ctx, const dca_pt_args* args, uint8_t* out /* M*R x L */, int32_t* levels_out /* M*R */,
                           double* energies_out /* M*R or NULL: E of the final codes */, uint64_t* attempts_out,
                           uint64_t* accepts_out /* R-1 each, or NULL */, double* energy_trace_out /* rounds x M x R, or NULL */,
                           int* rounds_out /* or NULL */);
/* Inter-protein interaction energies of a model fitted on a concatenated alignment: sites [0, split)
 * are protein A (LA = split), sites [split, L) protein B (LB = L - LA).  XA: nA x LA codes, XB: nB x LB codes.  Group g (a
 * species) holds the rows offsets_a[g] .. offsets_a[g+1] of XA and offsets_b[g] .. offsets_b[g+1] of XB; the offsets (G + 1
 * each) are non-decreasing, start at 0 and end at nA and nB; a group may be empty on either side.  out: the concatenation of
 * the G row-major blocks nA_g x nB_g (sum_g nA_g * nB_g doubles); all-against-all is G = 1.
 * The rule, every term widened to double and no contraction.  For i < LA <= j, Jt_ij(a, b) is
 *   gauge 0: the stored J_ij(a, b) as dca_plm_energies reads it (the mean-field model is zero on the gap state);
 *   gauge 1: its zero-sum form over all q states, kept in double and never rounded back to the storage type:
 *            r(a) = (sum_b J(a, b)) / q, c(b) = (sum_a J(a, b)) / q, m = (sum_a r(a)) / q, every sum from 0.0 in ascending
 *            index, Jt = ((J - r(a)) - c(b)) + m.
 *   phi_m(j, b) = sum over i = 0 .. LA-1, ascending, of Jt_{i, LA+j}(a^m_i, b): one sequential double sum from 0.0;
 *   E(m, n)     = sum over j = 0 .. LB-1, ascending, of phi_m(j, b^n_j):        one sequential double sum from 0.0.
 * No fields enter.  Higher E is the more favourable pair (the sign of dca_plm_energies).  E(m, n) depends only on the model,
 * the split, the gauge and the two rows: the same bits in any grouping, batch, block split or call.
 * phi (LB x q doubles per A-row) and the device output are bounded at 1 GiB each by running blocks of A-rows one after
 * another (DCA_CROSS_PASS caps the rows of a block).
 * DCA_ERR_ARG: split outside [1, L-1], negative counts, G < 1, offsets NULL or malformed, gauge not 0 or 1, XA, XB or out NULL
 * with energies to form, a code >= q; no energies to form is DCA_OK.  DCA_ERR_STATE: before dca_plm_configure; under column
 * strips, vector sharding, a reduce / comm hook or a native-comm mode (one GPU only, like dca_plm_sample_conditional).  An
 * L-BFGS or Boltzmann-learning run in progress is allowed; the alignment, the weights, x, g, the optimiser and the bmDCA chains
 * are not touched.  Profiling tags: "cross_fields" (phi, one launch per block), "cross_energy" (the pairs, one launch per
 * block).  No reference counterpart. */
int dca_plm_interaction_energies(dca_ctx* ctx, int split /* LA */, const uint8_t* XA /* nA x LA */, int nA,
                                 const uint8_t* XB /* nB x LB */, int nB, const int32_t* offsets_a /* G+1 */,
                                 const int32_t* offsets_b /* G+1 */, int G, int gauge /* 0: as stored, 1: zero-sum */,
                                 double* out /* sum_g nA_g * nB_g */);
/* The same under the mean-field model (J as in dca_mf_energies; zero on the gap state).  DCA_ERR_STATE before
 * dca_mf_couplings. */
int dca_mf_interaction_energies(dca_ctx* ctx, int split, const uint8_t* XA, int nA, const uint8_t* XB, int nB,
                                const int32_t* offsets_a, const int32_t* offsets_b, int G, int gauge, double* out);
/* Maximum-weight matching of size min(nr, nc) in the nr x nc matrix E (row-major; rectangular allowed) by shortest augmenting
 * paths, on the host (no device, no context, no threads, deterministic).  col_of_row[r]: the column of row r, -1 if unassigned.
 * total_out (or NULL): the matching's total.  gap_out (or NULL; nr): for an assigned row, total - (the best total of a matching
 * of the same size that may not use (r, col_of_row[r])), >= 0, +inf where no such matching exists (a 1 x 1 block); 0 for an
 * unassigned row.  The gaps take one augmentation each from the optimal potentials.  Under exact ties any optimal matching may
 * come back (the total and the gaps are the same for all of them).  DCA_ERR_ARG: a negative size, a non-finite entry, E or
 * col_of_row NULL where needed; nr == 0 or nc == 0 is DCA_OK with total 0. */
int dca_assign_partners(const double* E, int nr, int nc, int32_t* col_of_row /* nr */, double* total_out, double* gap_out);
/* The counter-based generator of the samplers, on the host: Philox4x32-10 (Salmon et al., SC 2011; 10 rounds, multipliers
 * 0xD2511F53 / 0xCD9E8D57, key bumps 0x9E3779B9 / 0xBB67AE85).  Needs no device. */
int dca_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* coupling blocks of selected pairs, optionally gauge shifted (MeanFieldDCA.compute_params,
 * meanfield_dca.py:661-752; shift_couplings :636-658) */
int dca_mf_pair_couplings(dca_ctx* ctx, const int* pairs, int npairs, int shift, double* out);
/* Sequence sharding of the pair counts: with a hook set, every shard context (its block of the
 * alignment, the GLOBAL weights of those sequences via dca_set_weights) calls it once after its
 * local counts are on the device: g_dev = the Lq x Lq raw weighted counts (doubles), fx_dev = Meff
 * (one double); the hook sums both over the shards in place.  Everything downstream (frequencies,
 * correlation matrix, inverse, scores) is then identical on every shard. */
int dca_mf_set_reduce_hook(dca_ctx* ctx, dca_reduce_hook hook, void* user);
/* whole chain on the device: counts -> C -> -inv -> scores */
int dca_mf_run(dca_ctx* ctx, double pseudocount, int apc, double* scores_out, double* couplings_out /* may be NULL */);
/* stage API on caller-provided arrays: construct_corr_mat (:270-318) from regularised
 * frequencies (reg_fi: L*q, reg_fij: pairs*(q-1)^2) -> corr_out: (L(q-1))^2 */
int dca_mf_corr_from_freqs(dca_ctx* ctx, const double* reg_fi, const double* reg_fij, int L, int q, double* corr_out);
/* test hook / stage API: inverse of a host SPD matrix through the same device path */
int dca_spd_inverse(dca_ctx* ctx, const double* A, int n, double* Ainv_out);

/* ------------------------------------------------------------------ Hopfield-Potts model
 * Cocco, Monasson, Weigt, PLoS Comput Biol 9, e1003176 (2013).  With n = L (q - 1), C the matrix of dca_mf_corr_mat at the
 * context's weights and the given pseudocount and D its block diagonal, the patterns are the solutions of C u = lambda D u with
 * u^T D u = 1 (the entry of u of largest magnitude positive, ties to the smallest index).  A pattern's likelihood gain is
 * (lambda - 1 - ln lambda) / 2; it is attractive for lambda > 1 and repulsive for lambda < 1.  The couplings of the selected set
 * S are J = sum_S (1 - 1 / lambda) u u^T off the diagonal blocks, in the layout of dca_mf_couplings, and the fields are those of
 * dca_mf_fields on that J.
 * dca_mf_hopfield_fit: selection DCA_HOPFIELD_LIKELIHOOD takes the num_patterns patterns of largest gain over the whole spectrum
 * (equal gains go to the attractive side); DCA_HOPFIELD_EXPLICIT the num_attractive largest and num_repulsive smallest
 * eigenvalues.  Outputs, each of capacity p = num_patterns or num_attractive + num_repulsive, the attractive patterns first in
 * descending order of lambda, then the repulsive ones in ascending order: eigenvalues, gains, signs (+1 attractive: 1 - 1 /
 * lambda > 0; -1 repulsive), patterns (p x L (q - 1): xi = |1 - 1 / lambda|^1/2 u, so J = sum sign xi xi^T), residuals
 * (||Gamma v - lambda v|| with Gamma = R^-1 C R^-T, D = R R^T, v = R^T u, measured on Gamma itself for both ends).  Each end is
 * found by block subspace iteration with Rayleigh-Ritz on min(n, k + 8) vectors, the attractive end on Gamma and the repulsive end
 * on its inverse, until every wanted residual is <= tol * (the block's largest Ritz value) or max_iterations is reached; info
 * reports the iterations and the convergence of each end ([0] attractive, [1] repulsive) and how many patterns each gave.  The
 * order of every sum is fixed by the shapes alone: the same call gives the same bits.
 * Afterwards the context holds the Hopfield-Potts J: dca_mf_scores, dca_mf_di_scores, dca_mf_fields, dca_mf_pair_couplings and
 * every dca_mf_* sequence-model entry serve it until dca_mf_corr_mat, dca_mf_couplings, dca_mf_run, new weights or a new
 * exchange scheme return the context to the mean-field model.  dca_mf_model_kind tells which model is held;
 * dca_mf_hopfield_couplings copies J out (n x n; its diagonal blocks are as the sum gives them and mean nothing).
 * DCA_ERR_ARG: args or an output NULL, a selection that is neither, num_attractive or num_repulsive outside 0 .. 64, no pattern
 * or more than n asked for, a likelihood selection that needs more than 64 patterns of one end, tol <= 0, max_iterations < 1.
 * DCA_ERR_STATE: no alignment or weights; a row window, a reduce hook or a native communicator (one GPU only).
 * DCA_ERR_NOT_SPD: a diagonal block (the message names the site) or Gamma is not positive definite.
 * Profiling tags "hopfield_whiten", "hopfield_apply", "hopfield_assemble", "pca_small". */
#define DCA_HOPFIELD_EXPLICIT 0
#define DCA_HOPFIELD_LIKELIHOOD 1
#define DCA_MF_MODEL_NONE 0
#define DCA_MF_MODEL_MEAN_FIELD 1
#define DCA_MF_MODEL_HOPFIELD 2
typedef struct dca_hopfield_args {
    int32_t selection, num_patterns, num_attractive, num_repulsive, max_iterations;
    double tol;
    uint64_t seed;
} dca_hopfield_args;
typedef struct dca_hopfield_info { int32_t num_attractive, num_repulsive, iterations[2], converged[2]; } dca_hopfield_info;
int dca_mf_hopfield_fit(dca_ctx* ctx, double pseudocount, const dca_hopfield_args* args, double* eigenvalues_out, double* gains_out,
                        int32_t* signs_out, double* patterns_out, double* residuals_out, dca_hopfield_info* info_out);
int dca_mf_model_kind(dca_ctx* ctx, int* kind_out);
int dca_mf_hopfield_couplings(dca_ctx* ctx, double* out);
/* Overlaps of sequences with patterns: out[s * p + mu] = sum over the sites i ascending of xi_mu(i, s_i), a gap adding 0: one
 * chain of doubles per (sequence, pattern), so a sequence has the same bits alone, in any batch and under any DCA_NN_PASS (the
 * kernel and the passes of dca_pca_project).  Q: nq x L host codes, or NULL for the context's alignment; patterns: p x L (q - 1).
 * DCA_ERR_ARG: patterns or out NULL, p < 1, nq < 1 with Q, a code >= q.  DCA_ERR_STATE: no alignment. */
int dca_hopfield_project(dca_ctx* ctx, const uint8_t* Q, int nq, int p, const double* patterns, double* out);
/* test hook: Y (n x b) = A V for a host A (n rows at stride ld >= n) and a host V (n x b, 1 <= b <= 72) through the operator
 * kernel of the fit */
int dca_dense_apply(dca_ctx* ctx, const double* A, int n, int ld, const double* V, int b, double* Y);

/* ------------------------------------------------------------------ autoregressive model (arDCA)
 * Trinquier et al., Nat. Commun. 12, 5800 (2021).  Sites are in model order: the column order of the context's alignment (a
 * caller that wants another order permutes the columns before dca_set_msa).  x has the plm layout and size
 * (dca_ar_num_params == dca_plm_num_params): fields h_l(b) at l*q + b, then one q x q block per pair k < l in pair order
 * (0,1),(0,2)...,(1,2)..., element a*q + b = J_kl(a, b) with a the state of the EARLIER site k and b that of the later site l.
 * All q states are used, the gap q-1 included; everything is float64.
 *   u_l(b) = h_l(b) + sum_{k<l} J_kl(s_k, b)      (site 0: fields only)
 *   m_l = max_b u_l(b),  Z_l = sum_b exp(u_l(b) - m_l) (ascending b),  cond_l(b) = (u_l(b) - m_l) - log Z_l = log P(s_l = b | s_<l)
 *   log P(s) = sum_l cond_l(s_l) (ascending l)    -- exact: every conditional is normalised, no log Z is needed.
 * u_l is summed in double without contraction: h_l(b) first, then k ascending.  P_nl(b) = exp(cond_l(b)) of sequence n.
 * Objective of the fit, with W_n = w_n / sum_m w_m (the context's weights, dca_compute_weights / dca_set_weights):
 *   f(x) = -sum_n W_n log P(s_n) + lambda_h sum h^2 + lambda_J sum J^2                  (no gauge is fixed; the L2 term makes
 *   df/dh_l(b)    = sum_n W_n (P_nl(b) - [s_nl = b]) + 2 lambda_h h_l(b)                   the minimum unique)
 *   df/dJ_kl(a,b) = sum_n W_n [s_nk = a] (P_nl(b) - [s_nl = b]) + 2 lambda_J J_kl(a, b)
 * The sequences go through in passes that bound the device scratch (DCA_AR_PASS, a positive count, caps the pass size); the
 * sums over n ascend within a pass and the pass results are added in ascending pass order, so fx and g depend on (N, L, q, pass
 * size) and repeated calls give the same bits.  No float atomics.  Profiling tags "ar_logits", "ar_grad", "ar_sample".
 *
 * dca_ar_configure: lambdas finite and >= 0 (else DCA_ERR_ARG); DCA_ERR_STATE without an alignment or weights.  The first call
 * creates the engine with x = 0; later calls keep x.  A change of the weights unconfigures the engine (x stays): gradient and
 * fit answer DCA_ERR_STATE until the next dca_ar_configure.  The other entries need only x (DCA_ERR_STATE before the first
 * configure).  dca_ar_release frees the engine; dca_set_msa and dca_destroy free it too. */
#define DCA_AR_CONVERGED 0            /* |g| <= epsilon * max(1, |x|) */
#define DCA_AR_MAX_ITERATIONS 1       /* max_iterations reached */
#define DCA_AR_LINE_SEARCH_FAILED 2   /* the line search found no Wolfe point; x, fx and g are the last accepted point's */
typedef struct {
    int status;        /* DCA_AR_* */
    int iterations;    /* accepted L-BFGS steps */
    int evaluations;   /* objective/gradient evaluations, the initial one included */
    double fx, gnorm;  /* at the returned x */
    double seconds;
} dca_ar_stats;
int dca_ar_configure(dca_ctx* ctx, double lambda_h, double lambda_J);
size_t dca_ar_num_params(int L, int q);
int dca_ar_init_x(dca_ctx* ctx);                          /* x <- 0 */
int dca_ar_set_x(dca_ctx* ctx, const double* x);
int dca_ar_get_x(dca_ctx* ctx, double* x);
/* fx (fx_out may be NULL) and g at the current x; dca_ar_get_g reads g of the last evaluation */
int dca_ar_gradient(dca_ctx* ctx, double* fx_out);
int dca_ar_get_g(dca_ctx* ctx, double* g);
/* L-BFGS from the current x: memory m = 5, More-Thuente line search enforcing the strong Wolfe conditions (ftol 1e-4, gtol 0.9,
 * at most 20 evaluations), first step 1/|g| along -g, then 1.  Stops when |g| <= epsilon * max(1, |x|) (checked before the first
 * step too), after max_iterations accepted steps (0: evaluate only) or when the line search fails; stats_out (may be NULL) says
 * which.  Only scalars cross to the host.  DCA_ERR_ARG: max_iterations < 0, epsilon < 0 or not finite. */
int dca_ar_fit(dca_ctx* ctx, int max_iterations, double epsilon, dca_ar_stats* stats_out);
/* log P(s) of n query rows X (n x L codes < q, model order; host) under the current x.  Outputs (host): logp[n]; site[n*L]
 * (row n, site l at n*L + l: cond_l(s_l)) and cond[n*L*q] (at (n*L + l)*q + b) when not NULL.  A sequence's outputs have the
 * same bits whatever n, its position or the passes; logp is the ascending sum of its site values.  The alignment, weights, x
 * and g are not touched.  n == 0 is DCA_OK; a code >= q is DCA_ERR_ARG.  Profiling tag "ar_logits". */
int dca_ar_log_probabilities(dca_ctx* ctx, const uint8_t* X, int n, double* logp, double* site, double* cond);
/* Ancestral sampling of n exact, independent sequences under the current x.  Chain c = first_chain + k visits sites
 * l = 0 .. L-1 once: u_l(b) = (((h_l(b) + S_0(b)) + S_1(b)) + S_2(b)) + S_3(b), S_w(b) = sum over k < l, k = w (mod 4), ascending
 * k, of J_kl(s_k, b) (S_0 added onto h_l term by term); then dca_plm_sample's draw rule at beta = 1: p_b = exp(u_l(b) - m_l),
 * T = sum_b p_b ascending, r = U * T, s_l = the smallest b whose ascending cumulative sum exceeds r (the largest b with p_b > 0 if
 * rounding leaves none), U of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (chain, 0, l, 3).  out: n x L
 * codes (host, model order).  Chain k's codes depend only on x, seed and first_chain + k.  DCA_ERR_ARG: n < 0, out NULL with
 * n > 0, L > 10240; n == 0 is DCA_OK.  Profiling tag "ar_sample". */
int dca_ar_sample(dca_ctx* ctx, int n, uint64_t seed, uint64_t first_chain, uint8_t* out);
/* Double-mutant epistasis of the wild type w (L codes < q, model order; host) under the current x.  With w^{k->a} the wild type
 * with site k set to a (all q states, the gap included):
 *   d_k(a)       = log P(w^{k->a}) - log P(w)                                                   single_out[k*q + a]
 *   eps_kl(a, b) = log P(w^{k->a, l->b}) - log P(w^{k->a}) - log P(w^{l->b}) + log P(w),  k < l    eps_out[(pair*q + a)*q + b]
 * in pair order (0,1),(0,2)...,(1,2)..., a the state of the EARLIER site k; the double-mutant effect is d_k(a) + d_l(b) +
 * eps_kl(a, b).  No mutant sequence is formed: with cond_m the wild type's conditionals, p_m(c) = exp cond_m(c) and, for k < m,
 * U^k_m(a, c) = exp(J_km(a, c) - J_km(w_k, c)), S_m(k, a) = sum_c p_m(c) U^k_m(a, c), V^k_m(a, c) = U^k_m(a, c) / S_m(k, a):
 *   d_k(a)       = (cond_k(a) - cond_k(w_k)) + sum_{m>k} [(J_km(a, w_m) - J_km(w_k, w_m)) - log S_m(k, a)]   (m ascending)
 *   eps_kl(a, b) = T - log prod_{m>l} r_m,  r_m = sum_c (p_m(c) V^k_m(a, c)) V^l_m(b, c)          (c ascending, fused multiply-adds;
 *   T            = (J_kl(a, b) - J_kl(w_k, b)) - (J_kl(a, w_l) - J_kl(w_k, w_l))                   m ascending in the product)
 * The product's exponent is split off into an integer every 4th factor and one logarithm is taken at the end, so 4 consecutive
 * r_m may together span 2^+-1000.  The order of every sum depends on (L, q) alone: repeated calls, and calls with either or both
 * outputs, give the same bits.  Entries with a = w_k or b = w_l are 0.0 exactly, and d_k(w_k) = 0.0.  Either output may be NULL,
 * not both.  Device scratch: 2 L(L-1)/2 q^2 doubles (880 MB at L = 500, q = 21) from the context's pool; DCA_ERR_NOMEM when it
 * is not there.  The alignment, the weights, x and g are not touched.  DCA_ERR_ARG: wildtype NULL, a code >= q, both outputs
 * NULL; DCA_ERR_STATE before the first dca_ar_configure.  Profiling tag "ar_epistasis" (the wild-type pass: "ar_logits"). */
int dca_ar_epistasis(dca_ctx* ctx, const uint8_t* wildtype, double* eps_out /* pairs*q*q, may be NULL */,
                     double* single_out /* L*q, may be NULL */);
/* Contact scores from that table: eps as a plm-layout vector (L*q zero fields, then the pair blocks) through the path of
 * dca_plm_scores -- gap row and column dropped, the (q-1) x (q-1) block double-centred, Frobenius norm, APC-corrected with
 * apc != 0 -- in pair order over the MODEL's sites (FN and APC do not change under transposition of a block or relabelling of
 * the sites, so a caller with another site order relabels the pairs).  The score vector stays on the device for
 * dca_scores_order, as after dca_plm_scores; like it, any L >= 2 and every q of dca_set_msa is served.  Errors as
 * dca_ar_epistasis (scores_out NULL: DCA_ERR_ARG). */
int dca_ar_epistatic_scores(dca_ctx* ctx, const uint8_t* wildtype, int apc, double* scores_out /* pairs */);
int dca_ar_release(dca_ctx* ctx);

/* ------------------------------------------------------------------ comparing sequence sets with the alignment
 * Model-free: these entries use the context's alignment (and, for the comparison, its weights), never its parameters; the
 * alignment, the weights and any fitted model (plm, mf, ar, a Boltzmann run) stay untouched.  DESIGN.md section 17.
 *
 * Hamming distances between a query set and a reference set of aligned, encoded sequences (same table, same L).  L and q are
 * those of the context's alignment, so dca_set_msa comes first in every case (DCA_ERR_STATE otherwise); Q and R are host rows
 * (nq x L, nr x L codes < q; a larger code is DCA_ERR_ARG).
 * R == NULL: the reference set is the context's alignment (dca_set_msa), already on the device; nr is ignored.  Q == NULL: the
 * query set IS the reference set; nq is ignored.  skip_same_index != 0: the pairs (k, m) with k == m are left out (a set against
 * itself).  dist_out[k] = min_m d(Q_k, R_m); index_out[k] = the SMALLEST m that attains it; hist_out[d] = number of
 * compared pairs (k, m) at distance d, d = 0..L (so sum(hist) = nq*nr, or nq*nr - min(nq,nr) with skip_same_index).
 * index_out and hist_out may be NULL.  A query with no partner (nr == 1 and skipped) gets dist -1, index -1.
 * Everything is integer: the outputs do not depend on the batch a query is in, on the pass split (DCA_NN_PASS, a positive
 * count, caps the queries per pass) or on the launch geometry.  DCA_ERR_ARG: dist_out NULL, nq < 1 with Q, nr < 1 with R.
 * Profiling tag "hamming". */
int dca_hamming_nearest(dca_ctx* ctx, const uint8_t* Q, int nq, const uint8_t* R, int nr, int skip_same_index,
                        int32_t* dist_out, int32_t* index_out, uint64_t* hist_out);

typedef struct {           /* one block per quantity: [0] f_i, [1] f_ij, [2] c_ij (connected) */
    double pearson[3], slope[3], max_abs_diff[3];
    double sxx[3], syy[3], sxy[3];      /* the centred sums the three above are formed from; x = alignment, y = query set */
    double terms[3];                    /* number of terms: L*q, pairs*q*q, pairs*q*q */
} dca_set_comparison;

/* One- and two-site frequencies of nq encoded sequences (unweighted: count / nq, all q states), optionally returned
 * (fi_out: L*q; fij_out: pairs*q*q in pair order, either may be NULL), and their comparison with the context's
 * alignment under the context's sequence weights (dca_compute_weights / dca_set_weights first), no pseudocount.
 * Centred with the analytic means (1/q, 1/q^2, 0):  sxx = sum (x - mu)^2, syy, sxy over all terms, c_ij(a, b) = f_ij(a, b) -
 * f_i(a) f_j(b) of each side; pearson = sxy / sqrt(sxx syy) (0 when sxx syy <= 0), slope = sxy / sxx (0 when sxx == 0),
 * max_abs_diff = max |x - y|.  All in double, without contraction, in an order fixed by (L, q): no float atomics.
 * cmp_out may be NULL (frequencies only; no weights needed then).  DCA_ERR_ARG: Q NULL, nq < 1, a code >= q, all three outputs
 * NULL; DCA_ERR_STATE: no alignment, cmp_out without weights.  Profiling tags "bm_stats" (the counts), "set_compare". */
int dca_sequence_statistics(dca_ctx* ctx, const uint8_t* Q, int nq, double* fi_out, double* fij_out, dca_set_comparison* cmp_out);
/* The alignment's side of that comparison: the weighted frequencies of all q states, no pseudocount (fi_out: L*q, fij_out:
 * pairs*q*q in pair order; either may be NULL, not both) -- the x that dca_sequence_statistics compares with, bit for bit. */
int dca_alignment_statistics(dca_ctx* ctx, double* fi_out, double* fij_out);

/* Three-site connected correlations, the statistic no pairwise fit has seen:
 *   c_ijk(a,b,c) = f_ijk(a,b,c) - f_ij(a,b) f_k(c) - f_ik(a,c) f_j(b) - f_jk(b,c) f_i(a) + 2 f_i(a) f_j(b) f_k(c)
 * All three-site work is in integers.  Sequence n carries the weight wq_n = llrint(w_n * 2^40) for the alignment (Q == NULL; w_n
 * the context's double weights, the ones dca_alignment_statistics uses) and wq_n = 1 for a query set; the denominator is
 * M = sum_n wq_n (nq for a set).  Every count -- of a triple, and of the one- and two-site marginals that enter c_ijk -- is the
 * uint64 sum of wq over the matching sequences, a frequency is (double)count / (double)M, and c_ijk is formed in double, without
 * contraction, in exactly the order written, left to right, the last term as 2.0 * f_i * f_j * f_k.  So c_ijk sums to zero over
 * any of its three state indices up to rounding, and nothing depends on the launch geometry, the order of any atomic (all are
 * integer) or the pass split.  For a set f_i and f_ij are bit-equal to dca_sequence_statistics.  For the alignment the quantised
 * weights are a different, fully specified weighting: its f_i and f_ij differ from dca_alignment_statistics by at most
 * 2 N 2^-41 / Meff.  An alignment of more than 2^23 sequences, or a weight outside [0, 1] (dca_set_weights; the weights of
 * dca_compute_weights are 1 / count), is DCA_ERR_ARG: the sums stay below 2^63.
 *
 * dca_three_site_values: elements = T rows (i, j, k, a, b, c), i < j < k < L, states < q, in the context's column order; a row
 * may repeat.  Q == NULL: the context's alignment under its quantised weights; else nq x L host codes with unit weights, uploaded
 * in passes of at most DCA_NN_PASS queries (the variable of dca_hamming_nearest; integers make the split invisible).
 * count_out (uint64[T]), denom_out (uint64*), f3_out, c3_out (double[T]) may each be NULL, not all.
 *
 * dca_three_site_scan: the K elements of largest |c_ijk(a,b,c)| over ALL site triples i < j < k and all states (states equal to
 * skip_state left out of a, b and c; -1: none), of the alignment (Q == NULL) or of a set.  Sorted by |c| descending, ties by
 * ascending (i, j, k, a, b, c).  *found = min(K, number of eligible elements); elements_out holds K rows of 6, c3_out and f3_out
 * (either may be NULL) K values.  The scan tiles the later sites (j, k) in TB x TB blocks, TB the largest of 8, 4, 2 with
 * TB^2 q^2 <= 7168 (q = 5: 8, q = 21: 4, q = 32: 2); the result does not depend on it.  Exact, with device memory O(K) beyond the
 * pair table: a histogram pass over the high bits of |c|, at most one refinement of the bin that holds the K-th value, and an
 * append pass whose buffer the histogram sized.  If more than 16 K + 2^20 elements still tie with the K-th value (for instance
 * K reaches into exact zeros of a large alignment) the call is DCA_ERR_ARG with a message instead of allocating without bound
 * (DCA_THREE_SITE_CAP, a positive count read per call, replaces that cap).
 *
 * DCA_ERR_STATE: no alignment; weights missing with Q == NULL.  DCA_ERR_ARG: L < 3, K < 1, T < 1, nq < 1 with Q, an index out of
 * order or out of range, a code >= q, a NULL context.  Profiling tags "three_site_scan" (one launch per pass), "three_site_values".
 * No reference counterpart. */
int dca_three_site_values(dca_ctx* ctx, const uint8_t* Q, int nq, const int32_t* elements, int T,
                          uint64_t* count_out, uint64_t* denom_out, double* f3_out, double* c3_out);
int dca_three_site_scan(dca_ctx* ctx, const uint8_t* Q, int nq, int K, int skip_state,
                        int32_t* elements_out, double* c3_out, double* f3_out, int* found);

/* Principal components of the reweighted alignment and projections of sequence sets onto them.
 * With x_n the L q one-hot row of sequence n (all q states, the gap included, columns in the context's order), w_n the context's
 * double weights and Meff = sum_n w_n:  f(i,a) = sum_n w_n [s_ni = a] / Meff,  C = sum_n w_n (x_n - f)(x_n - f)^T / Meff  (L q x
 * L q; its blocks are f_ij - f_i f_j^T, the diagonal blocks included; never formed), total_variance = trace C = sum_i (1 -
 * sum_a f(i,a)^2).
 *
 * dca_pca_fit: the k largest eigenpairs (lambda_m, v_m) of C, lambda descending, ||v_m|| = 1, the entry of v_m of largest
 * magnitude positive (ties: the smallest index); components_out holds v_m at [m * L q + i q + a].  offsets_out[m] = c_m = sum
 * over (i,a) ascending of f(i,a) v_m(i,a), one double chain.  Block subspace iteration with Rayleigh-Ritz on b = min(L q, k + 8)
 * vectors whose start is a function of (seed, element) alone; one iteration applies C to the block by two passes over the code
 * bytes.  residuals_out[m] = ||C v_m - lambda_m v_m|| as the last iteration evaluated it; the fit is converged (*converged_out
 * = 1) when every one of the k is <= tol * lambda_1.  Out of iterations: DCA_OK with *converged_out = 0 and the residuals.  A
 * component with lambda_m <= tol * lambda_1 is NULL: eigenvalue 0, an all-zero vector and offset (rank C < k, one sequence, a
 * constant alignment; a trace of at most 4 L 2^-52 counts as C = 0 and returns k null components after 0 iterations).
 * No float atomics; every sum runs in an order fixed by (N, L, q, b): the back-projection walks slabs of DCA_PCA_SLAB sequences
 * in ascending order and adds the slabs ascending, so two calls with the same arguments return the same bits.
 * residuals_out, total_variance_out and iterations_out may be NULL.
 *
 * dca_pca_project: proj_out[n * k + m] = (sum over the sites i ascending of v_m(i, s_ni)) - c_m: one double chain, then one
 * subtraction, no contraction -- a pure function of (v_m, c_m, s_n), so a sequence has the same bits alone, in any batch and
 * under any pass split.  Q == NULL: the context's alignment (nq ignored); else nq x L host codes, uploaded in passes of at most
 * DCA_NN_PASS rows (the variable of dca_hamming_nearest).  components (k * L q) and offsets (k) are host arrays as dca_pca_fit
 * returns them; any k >= 1 values are taken as given.
 *
 * Both are model-free and stateless: the alignment, the weights and any fitted model stay untouched; one GPU.
 * DCA_ERR_STATE: no alignment; no weights (dca_pca_fit).  DCA_ERR_ARG: k < 1, k > min(64, L q) (dca_pca_fit), tol <= 0,
 * max_iterations < 1, a NULL output or input, nq < 1 with Q, a code >= q, a NULL context.  Profiling tags "pca_project",
 * "pca_back" (the slab sums and their reduction), "pca_small" (b x b products and rotations).  No reference counterpart. */
#define DCA_PCA_SLAB 1024
int dca_pca_fit(dca_ctx* ctx, int k, double tol, int max_iterations, uint64_t seed,
                double* eigenvalues_out /* k */, double* components_out /* k*L*q */, double* offsets_out /* k */,
                double* residuals_out /* k, may be NULL */, double* total_variance_out /* may be NULL */,
                int* iterations_out /* may be NULL */, int* converged_out);
int dca_pca_project(dca_ctx* ctx, const uint8_t* Q, int nq /* Q == NULL: the context's alignment */, int k,
                    const double* components /* k*L*q, host */, const double* offsets /* k */, double* proj_out /* nq*k */);

/* ------------------------------------------------------------------ redundancy filter and identity clusters
 * Preprocessing of a raw alignment: model-free and stateless, the alignment, the weights and any fitted
 * model stay untouched; one GPU.  L and q are those of the context's alignment, so dca_set_msa comes first (DCA_ERR_STATE
 * otherwise).  X: n x L host codes < q, or NULL: the context's alignment, already on the device (n is ignored).
 *
 * ident(m, n) = #{i : X_mi = X_ni}, the gap state counting like any other (as dca_compute_weights counts it).  Two rows are
 * SIMILAR iff ident >= min_identical, an integer number of sites in 1 .. L + 1 (L + 1: nothing is similar to anything, not
 * even a row to itself).  No floating-point rule enters: the caller turns an identity fraction into the count.
 *
 * dca_identity_filter: the sequential greedy filter.  order (n entries, a permutation of 0 .. n-1; NULL: ascending row index)
 * gives the priority; rows are visited in that order and a row is KEPT iff no row kept before it is similar to it.
 * keep_out[r] = 1 / 0; rep_out[r] = r for a kept row, else the kept row similar to r that comes EARLIEST IN THE ORDER.  The
 * device returns exactly that: blocks of rank positions (DCA_FILTER_BLOCK, a positive count read per call, rounded up to a
 * multiple of 64, at most 8192; 2048 when unset) are compared with the compact list of the rows kept so far (a 32-bit unsigned
 * atomicMin of rank positions: a minimum, so arrival order cannot show) and resolved in ascending order by one workgroup; the
 * count of kept rows stays on the device between blocks and the call synchronises once, at its end.  The result does not
 * depend on the block size.  info (may be NULL): kept = number of kept rows, blocks and block_rows = the block plan,
 * tile_pairs = the 64 x 64 tiles the launches covered (the cover pass is launched for the worst case).
 *
 * dca_identity_clusters: the connected components of the graph of similar pairs (single linkage).  label_out[r] = the SMALLEST
 * row index of r's component; degree_out[r] (may be NULL) = #{m : ident(r, m) >= min_identical}, r itself included -- with the
 * strict threshold of dca_compute_weights these are the integers of dca_get_weight_counts.  The n x ceil(n / 32)-dword
 * similarity matrix stays on the device while n * ceil(n / 32) * 4 bytes <= DCA_CLUSTER_BITS_MAX (bytes, read per call; 8 GiB
 * when unset); above it every round recomputes the compares from the bit planes and nothing is stored.  Both paths return the
 * same labels and degrees.  Rounds of hook (atomicMin on labels) and pointer jumping repeat until one passes without a change;
 * the fixpoint is unique (every label its component's smallest index), so the atomics' order cannot show.  info (may be NULL):
 * clusters = number of components, largest = rows of the largest, rounds = rounds run (the last, unchanged one included),
 * stored_bits = 1: the bits were kept, 0: recomputed per round.
 *
 * DCA_ERR_ARG: a NULL context, keep_out / label_out NULL, n < 1 with X, a code >= q, min_identical outside 1 .. L + 1, an order
 * that is not a permutation.  Profiling tags "identity_filter", "identity_clusters" (the whole call; its parts under
 * "identity_clusters_bits", "identity_clusters_degrees", "identity_clusters_rounds").  No reference counterpart. */
typedef struct { int32_t kept, blocks, block_rows; int64_t tile_pairs; } dca_filter_info;
typedef struct { int32_t clusters, largest, rounds, stored_bits /* 1: adjacency kept as bits, 0: recomputed per round */; } dca_cluster_info;

int dca_identity_filter(dca_ctx* ctx, const uint8_t* X /* n x L, or NULL: the context's alignment */, int n, int min_identical,
                        const int32_t* order /* n, or NULL */, uint8_t* keep_out /* n */, int32_t* rep_out /* n, may be NULL */,
                        dca_filter_info* info /* may be NULL */);
int dca_identity_clusters(dca_ctx* ctx, const uint8_t* X, int n, int min_identical, int32_t* label_out /* n */,
                          int32_t* degree_out /* n, may be NULL */, dca_cluster_info* info /* may be NULL */);

/* ------------------------------------------------------------------ timing
 * When profiling is on, selected kernels are bracketed with HIP events on the
 * context's stream.  dca_get_kernel_time returns accumulated ms and launch count
 * for a kernel tag ("weights", "plm_logits", "plm_softmax", "plm_scatter", "plm_expand",
 * "plm_fold", "lbfgs_vec", "mf_counts", "mf_inverse", "scores", "energies", "mutation_scan", "pll", "sample", "cond_fields", "sample_cond", "ar_logits", "ar_grad", "ar_sample", "ar_epistasis",
 * "bm_stats", "bm_decimate", "gauge", "ais", "hamming", "set_compare", "three_site_scan", "three_site_values", "pca_project", "pca_back", "pca_small",
 * "identity_filter", "identity_clusters"). */
int dca_set_profiling(dca_ctx* ctx, int on);
/* Only the stage of this name ("plm_scatter", "plm_logits", "mf_inverse", ...) is bracketed -- two event records per launch of it
 * instead of two per stage (an event record costs the stream ~5 us: 14 per plmDCA iteration are 5 % of config C's step, 0.4 % of
 * D's).  NULL or "" switches profiling off.  Measurement aid of bench.py's timed region; no reference counterpart. */
int dca_set_profiling_only(dca_ctx* ctx, const char* stage);
int dca_get_kernel_time(dca_ctx* ctx, const char* tag, double* ms_out, int* launches_out);
int dca_reset_kernel_times(dca_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DCA_HIP_H */
