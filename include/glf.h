/*
 * glf.h -- C-ABI of the MI355X-native graph-Laplacian image filter.
 *
 * Drop-in boundary for the approximate path of the reference program
 * hpc/image_processing (David-Wobrock/image-processing-graph-laplacian).
 * The reference has no FFI; its boundary is the per-stage C prototypes in
 * the hpc/ headers, all of which take PETSc Mat/Vec. Here Mat/Vec become flat HIP
 * device buffers described by the plain struct glf_mat; every entry point is
 * extern "C", takes plain pointers and sizes, and returns an int status
 * (0 = GLF_OK) instead of void. Each declaration cites the reference
 * interface it replaces (paths relative to the reference root).
 *
 * Layout conventions (all device matrices are float32, ROW-major):
 *   image        uint8  [height][width]            (x = idx / width is the row,
 *                                                   y = idx % width the column, hpc/utils.c:11-19)
 *   K_A, L_A     float  [p][lda]  lda = p rounded up to 64, zero padding (the eigen stages need it)
 *   X, Phi_A     float  [p][ld]   ld = m rounded up to 32, columns >= m are zero
 *   Phi          float  [N][ld]   row order GLF_ROWS_SAMPLE_FIRST or GLF_ROWS_RASTER
 *   K_B, L_B     never stored: a GLF_MAT_KERNEL_B descriptor (image + sample table + scale)
 *
 * Threading: one host thread drives one context; contexts are independent.
 * Multi-GPU: pixel rows are sharded over the ranks (see glf_image_processing); a rank is one GPU. The collectives
 * are RCCL calls issued by the library itself (glf_ctx_set_comm_rccl: one process per GPU; glf_multi_*: one process,
 * one thread per GPU), or callbacks the caller plugs in through glf_comm.
 */
#ifndef GLF_H
#define GLF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLF_VERSION 100

/* ---- status codes ---------------------------------------------------------- */
enum {
    GLF_OK = 0,
    GLF_ERR_INVALID = -1,   /* bad argument / shape mismatch */
    GLF_ERR_NOMEM = -2,     /* hipMalloc / malloc failed */
    GLF_ERR_HIP = -3,       /* a HIP call or kernel launch failed */
    GLF_ERR_NODEVICE = -4,  /* no usable gfx950 device */
    GLF_ERR_COMM = -5,      /* a glf_comm callback failed */
    GLF_ERR_NOCONV = -6,    /* eigensolver hit max_outer / inner limit */
    GLF_ERR_IO = -7,        /* read_png / write_png */
    GLF_ERR_UNSUPPORTED = -8
};
const char *glf_strerror(int status);

/* ---- context ---------------------------------------------------------------- */
typedef struct glf_ctx glf_ctx; /* opaque: device, stream, workspace, comm */

/* Replaces InitProgram (hpc/image_processing.c:30-38: SlepcInitialize/MPI).
 * stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL
 * for a stream owned by the context. */
int glf_ctx_create(glf_ctx **ctx, int device, void *hip_stream);
int glf_ctx_destroy(glf_ctx *ctx);      /* replaces SlepcFinalize, :332 */
int glf_ctx_synchronize(glf_ctx *ctx);
const char *glf_ctx_last_error(const glf_ctx *ctx);
/* Device name / CU count / memory, for reports. */
int glf_ctx_device_info(const glf_ctx *ctx, char *name, size_t name_len, int *num_cus,
                        size_t *total_mem_bytes);
/* Kernel selection. Several stages have more than one implementation of the same sums (grid-factored vs entry by entry, two
 * row-pass shapes, ...); the default picks by problem size. key / value (value NULL, "" or "auto" = default):
 *   NYS_PATH  band | rank | grid | direct     DEG_PATH  grid | direct     MV_PATH  band | rank | grid | dense
 *   ROWPASS, ROWPASS_OP  rt | v1     COLPASS  ws | v1     SWEEP_COLPASS  segments | samples
 *   NYS_NO_LUT, NO_ECR, NO_NARROW, NO_FUSED_FILTER, BAND_NOSKIP, ZMFMA_GROUPS, VERBOSE  1 | 0     EIG_SHARD  1 | 0       GS        seq | gram          RESIDUAL  sweep | derived
 *   FILTER_FORM  sep | vec | phi (default: sep where it applies, else vec, else phi): the filter fused into the band-form Nystroem
 *     launch is contracted with q = Psi w, one column per plane, in separable form with the photometric table as a rank-R expansion
 *     (k_band_sep_*: a row pass and a column pass; needs an expansion of at most 48 terms, stats rank_terms = R), pair by pair
 *     with the exact table (k_band_vec; rank_terms = 0), or taken from the 64 columns of Phi in k_band's epilogue (also where the
 *     window of samples of the vec form does not fit the LDS). Same conditions for fusing, same stats keys; nystroem_mfma_flops = 0
 *     under sep and vec.
 *   PIX_BAND  1 | 0 (default 0): the colour, 16-bit, float and float colour bilateral kernels (GLF_KERNEL_BILATERAL_RGB / _U16 / _F32 / _RGBF32) take the band form of
 *     the Nystroem stage and of the L_A operator under exactly the conditions under which the grey kernel takes it -- split-f16
 *     contraction, a tensor-grid sample set, at most 64 eigenpairs, the radius and band-row limits, NYS_PATH auto (width >= 1024)
 *     or band, MV_PATH auto (p >= 16 384) or band -- with the photometric factor generated per entry (one v_exp_f32) instead of
 *     gathered from the 256-level table. L_A is then neither built nor stored. The degree stage and the filter stage are
 *     unchanged (entry by entry; Phi is written, filter_fused = 0). Wherever the form does not apply, and with the key off, the
 *     entry-by-entry route runs, bit for bit as before. The grey kernels never read the key.
 * At context creation each key is initialised from the environment variable GLF_<KEY> (read once; nothing reads the
 * environment per call). No reference counterpart (PETSc's -ksp_type / -pc_type options database is the nearest thing). */
int glf_ctx_set_tuning(glf_ctx *ctx, const char *key, const char *value);
/* Debug workspace pool (environment GLF_POOL_DEBUG=1 at context creation; no reference counterpart): every work
 * buffer is allocated at its exact size followed by a 4 KiB guard zone of canary bytes, floating-point buffers are
 * handed out filled with NaN instead of whatever an earlier call left in them, nothing is reused, and the guard is
 * verified when the buffer is released. Returns the number of guard zones found overwritten so far (0 = no kernel
 * wrote past the end of a work buffer), -1 when the context was not created in debug mode. */
int glf_ctx_debug_violations(const glf_ctx *ctx);
/* Work buffers are cached between calls (a second image of the same size allocates nothing). Bytes currently cached and not
 * in use; a cached buffer that no call has taken for 64 public calls is returned to the driver at the next allocation, so a
 * process that walks through many image sizes does not keep every size's buffers. No reference counterpart. */
size_t glf_ctx_cached_bytes(const glf_ctx *ctx);

/* Collectives supplied by the caller (replace the MPI_Allreduce / allgather
 * inside PETSc's VecDot, VecSum, MatMult: hpc/gram_schmidt.c:14-15,
 * hpc/utils.c:382, hpc/inverse_power_it.c:167). Buffers are DEVICE pointers,
 * operated in place, ordered on the context's stream. size == 1 or NULL
 * callbacks mean "single GPU". Return 0 on success. */
typedef struct glf_comm {
    int rank, size;
    int (*allreduce_sum_f32)(void *user, float *dbuf, size_t count);
    int (*allreduce_sum_f64)(void *user, double *dbuf, size_t count);
    /* In-place all-gather: dbuf holds size * count_per_rank floats, rank r's block at offset
     * r * count_per_rank (replaces the allgather inside PETSc's MPIDENSE MatMult). Optional: with
     * NULL the eigen-solve is replicated on every rank instead of row-sharded. */
    int (*allgather_f32)(void *user, float *dbuf, size_t count_per_rank);
    void *user;
} glf_comm;
int glf_ctx_set_comm(glf_ctx *ctx, const glf_comm *comm);

/* ---- native collectives: RCCL inside the library ------------------------------------------------------------------
 * The reference is an MPI program (hpc/image_processing.c:30-38 SlepcInitialize/MPI_Init, :45-76 broadcast of the image;
 * every Mat is MATMPIDENSE, hpc/affinity.c:138-142). Here a rank is a GPU and the collectives are RCCL calls the library
 * issues on the context's stream -- no callback into the host language on the data path:
 *   all-reduce (f64)  degree partial sums (p), Phi^T y (ld), every inner product / norm / Gram block of the eigen-solve
 *   all-reduce (f32)  X^T A X of the residual (ld x ld)
 *   all-gather (f32)  the operand block of each L_A application (hpc/inverse_power_it.c:167: PETSc's MPIDENSE MatMult
 *                     gathers x the same way) and the final eigenvectors
 * One process per GPU: glf_rccl_unique_id on one rank, distribute the bytes (MPI / torch.distributed / a file), then
 * glf_ctx_set_comm_rccl on every rank (ncclCommInitRank; collective over all ranks). force != 0 keeps the collectives
 * in place on a one-rank world (plumbing test on a single GPU). */
#define GLF_RCCL_ID_BYTES 128
int glf_rccl_unique_id(void *id_out, size_t bytes);
int glf_ctx_set_comm_rccl(glf_ctx *ctx, int rank, int size, const void *unique_id, size_t bytes, int force);

/* One PROCESS driving n GPUs -- the reference's `mpirun -n N image_processing` as `image_processing -ngpu N`: one
 * context and one host thread per device. GLF_MULTI_RCCL: ncclCommInitAll over `devices` (distinct GPUs of one node,
 * xGMI). GLF_MULTI_LOOPBACK: the same collectives staged through host memory between the rank threads in fixed rank
 * order; ranks may share a device (devices[i] may repeat), which RCCL refuses -- this is how the N > 1 sharding of the C
 * path is tested on a one-GPU box. devices == NULL: 0 .. n-1. */
/* info = {rank, size, backend (0 none / caller's callbacks, 1 RCCL, 2 loopback), ranks the RCCL communicator itself reports
 * (ncclCommCount; 0 when not RCCL)} */
int glf_ctx_comm_info(glf_ctx *ctx, int info[4]);
/* collectives issued through the library's own communicator since the last reset:
 * out = {all-reduce calls, all-reduce bytes, all-gather calls, all-gather bytes received} */
int glf_ctx_comm_counters(glf_ctx *ctx, unsigned long long out[4], int reset);

typedef struct glf_multi glf_multi;
enum { GLF_MULTI_RCCL = 0, GLF_MULTI_LOOPBACK = 1 };
int glf_multi_create(glf_multi **w, int n, const int *devices, int backend);
int glf_multi_destroy(glf_multi *w);
int glf_multi_size(const glf_multi *w);
glf_ctx *glf_multi_ctx(glf_multi *w, int rank);
const char *glf_multi_last_error(const glf_multi *w);
/* glf_multi_image_processing: declared below, after glf_options / glf_stats. */

/* How the Nystroem contraction L_B^T (phi_A Pi^-1) (hpc/nystroem.c:42) is evaluated:
 *  F32_MFMA   v_mfma_f32_32x32x2_f32, operands exactly f32 (shares the f32 FMA pipe with the
 *             kernel generation: about 75 % of the f32 matrix peak);
 *  F16_SPLIT  both operands split into f16 (hi, lo) pairs carrying 22 significant bits, three
 *             v_mfma_f32_32x32x16_f16 products, f32 accumulation; runs on the f16 matrix pipe so the
 *             MFMAs overlap the VALU generation (2.5x faster). Default; override per context here or
 *             with the environment variable GLF_CONTRACTION=f32|f16s at context creation. */
enum { GLF_CONTRACT_F32_MFMA = 1, GLF_CONTRACT_F16_SPLIT = 2 };
int glf_ctx_set_contraction(glf_ctx *ctx, int mode);
/* The pixel-row shard of rank `rank` of `size`: rows [*row0, *row1) = [rank*height/size, (rank+1)*height/size).
 * Host only (replaces PETSc's PETSC_DECIDE row ownership, hpc/utils.c:463-475). */
int glf_shard_rows(int height, int rank, int size, int *row0, int *row1);
/* Band form of the Nystroem extension (NYS_PATH band), host only: the schedule its kernel runs for the image rows
 * [row_begin, row_end) of a width x height image whose samples are the tensor grid rows[nr] x cols[nc] (ascending), with the
 * spatial scale h_loc. Workgroups take GLF_BAND_WG_ROWS consecutive target rows from row_begin on, one wave per row and tile of
 * *tile_px target columns; a workgroup pairs the grid rows within the radius of its target rows from the first one on, and a
 * wave executes, per pair, an interval of half-blocks (8 consecutive sample columns: column index >> 3). Outputs, each may be NULL:
 *   *rad the radius in pixels, *tile_px, *ntiles = ceil(width / *tile_px)
 *   first_row[r - row_begin]                                 first grid row of the band of r's workgroup (-1: no band)
 *   units[((r - row_begin) * ntiles + t) * pair_stride + j]  lo | hi << 16: the half-blocks the wave of (r, t) executes of grid
 *                                                            rows first_row + 2 j and + 2 j + 1; lo > hi: none
 *   *ksteps  the MFMA k-steps of the launch: the sum of the intervals' lengths (x 16 x *tile_px = nystroem_evaluated)
 * GLF_ERR_UNSUPPORTED: radius beyond what the kernel's tables hold; GLF_ERR_INVALID: a band of more than pair_stride pairs. */
enum { GLF_BAND_WG_ROWS = 8 };
int glf_band_plan(const int *rows, int nr, const int *cols, int nc, float h_loc, int width, int height, int row_begin, int row_end,
                  int pair_stride, int *rad, int *tile_px, int *ntiles, int *first_row, unsigned *units, uint64_t *ksteps);

/* Flat device buffers (replace MatCreate/VecCreate + MatDestroy/VecDestroy). */
int glf_malloc(glf_ctx *ctx, void **dptr, size_t bytes);
int glf_free(glf_ctx *ctx, void *dptr);
int glf_memcpy_h2d(glf_ctx *ctx, void *dst, const void *src, size_t bytes);
int glf_memcpy_d2h(glf_ctx *ctx, void *dst, const void *src, size_t bytes);
int glf_memset(glf_ctx *ctx, void *dst, int value, size_t bytes);

/* ---- matrices ----------------------------------------------------------------- */
enum { GLF_MAT_DENSE = 0, GLF_MAT_DIAG = 1, GLF_MAT_KERNEL_B = 2 };
enum { GLF_ROWS_NA = 0, GLF_ROWS_SAMPLE_FIRST = 1, GLF_ROWS_RASTER = 2 };
/* NLM: non-local means, 7 x 7 Gaussian-weighted patches of the symmetrically padded image, K = exp(-|| G o (P_i - P_j) ||^2 / h_val^2)
 * (python/affinity_methods/NLM.py:9-34, where h = 3; the C reference has bilateral / photometric / spatial only, hpc/affinity.c:8-121) */
/* BILATERAL_RGB: the colour bilateral kernel K = exp(-(dr^2 + dc^2) / h_loc^2) exp(-(dR^2 + dG^2 + dB^2) / h_val^2), i.e. the
 * photometric factor once per channel. With it the stage entry points (glf_ComputeAffinityMatrices and every consumer of its
 * KERNEL_B descriptor) read d_img as interleaved uint8 [height][width][3], the layout of glf_read_png_rgb. h_loc and h_val keep
 * their per-channel meaning: a grey image replicated into three channels gives the grey graph at h_val * sqrt(3). It has no
 * grid-factored, rank or band form: the entry-by-entry kernels run (f32 MFMA contraction whatever glf_ctx_set_contraction says). */
/* BILATERAL_U16: the bilateral kernel on 16-bit grey values, K = exp(-(dr^2 + dc^2) / h_loc^2) exp(-(v_i - v_j)^2 / h_val^2) with
 * v in 0..65535. With it the stage entry points (glf_ComputeAffinityMatrices and every consumer of its KERNEL_B descriptor) read
 * d_img as uint16_t [height][width] (glf_mat.img stays a byte pointer: the kernel id says how it is read). h_val is in the units
 * of the image's values on every entry point: an image 257 g (g an 8-bit image) at h_val * 257 has the graph of g at h_val. Like
 * the colour kernel it has no grid-factored, rank or band form (those factor over 256 grey levels): the entry-by-entry kernels run
 * with the f32 MFMA contraction whatever glf_ctx_set_contraction says. */
/* BILATERAL_F32: the same kernel on 32-bit float values, K = exp(-(dr^2 + dc^2) / h_loc^2) exp(-(v_i - v_j)^2 / h_val^2) with v any
 * finite float (negative and fractional included) and h_val in the image's own units. With it the stage entry points read d_img as
 * float [height][width]; an image with a NaN or an Inf is refused (GLF_ERR_INVALID). Routes and contraction as for BILATERAL_U16. */
/* BILATERAL_RGBF32: the colour kernel on float channels, K = exp(-(dr^2 + dc^2) / h_loc^2) exp(-((dR)^2 + (dG)^2 + (dB)^2) / h_val^2)
 * on an interleaved float [height][width][3] image of any finite values (HDR, [0, 1]-normalised RGB, Lab / YUV with negative chroma),
 * h_val in the image's units; a grey image replicated into three channels gives the grey graph at h_val * sqrt(3). With it the stage
 * entry points read d_img as float [height][width][3], and the sample descriptor (glf_mat.samples) carries one float4 {R, G, B, 0} per
 * sample behind its padded records. An image with a NaN or an Inf is refused (GLF_ERR_INVALID). Routes and contraction as for
 * BILATERAL_RGB: the entry-by-entry kernels (f32 MFMA contraction), and the band form behind PIX_BAND. */
enum { GLF_KERNEL_BILATERAL = 0, GLF_KERNEL_PHOTOMETRIC = 1, GLF_KERNEL_SPATIAL = 2, GLF_KERNEL_NLM = 3, GLF_KERNEL_BILATERAL_RGB = 4,
       GLF_KERNEL_BILATERAL_U16 = 5, GLF_KERNEL_BILATERAL_F32 = 6, GLF_KERNEL_BILATERAL_RGBF32 = 7 };

/* Replaces PETSc Mat (MATMPIDENSE / MATMPIAIJ diagonal). */
typedef struct glf_mat {
    int32_t kind;        /* GLF_MAT_* */
    int32_t row_order;   /* GLF_ROWS_* for N x m eigenvector matrices */
    int64_t rows, cols;  /* logical shape */
    int64_t ld;          /* floats between consecutive rows (DENSE) */
    float *data;         /* device; DENSE: rows*ld floats; DIAG: rows floats; KERNEL_B: NULL */
    int32_t owns_data;   /* glf_mat_destroy frees data */
    /* generator descriptor (KERNEL_B): entry (i, col) = scale * K(sample i, pixel col) */
    const uint8_t *img;  /* device image */
    const float *samples;/* device float4 per sample: {row, col, value, 0}, zero-padded to 64 records */
    const uint8_t *mask; /* device uint8[N]: 1 at sample pixels */
    const uint32_t *idx; /* device sample indices, ascending */
    int32_t width, height;
    uint32_t p;
    float scale;         /* 1 for K_B, -alpha for L_B (hpc/laplacian.c:37-38) */
    float h_loc, h_val;  /* hpc/affinity.c:117-118 */
    int32_t kernel;      /* GLF_KERNEL_* (hpc/affinity.c:119-121) */
    double *degree;      /* device double[p]: row sums of [K_A K_B] cached by
                            glf_ComputeAffinityMatrices (hpc/laplacian.c:18-20) */
    int32_t owns_desc;   /* glf_mat_destroy frees samples/mask/idx/degree */
} glf_mat;

int glf_mat_create_dense(glf_ctx *ctx, glf_mat *mat, int64_t rows, int64_t cols, int64_t ld);
int glf_mat_create_diag(glf_ctx *ctx, glf_mat *mat, int64_t n);
int glf_mat_destroy(glf_ctx *ctx, glf_mat *mat); /* MatDestroy */
/* MatGetColumnVector (hpc/display.c:95): column `col` of a dense matrix into host_out[rows]. */
int glf_mat_get_column(glf_ctx *ctx, const glf_mat *mat, int64_t col, float *host_out);

/* ---- host-side stages -------------------------------------------------------- */

/* void Sampling(int, int, unsigned*, unsigned**)  hpc/sampling.h:1, hpc/sampling.c:6-33.
 * *sample_indices is malloc'd; release with glf_host_free. */
int glf_Sampling(int width, int height, unsigned *sample_size, unsigned **sample_indices);
void glf_host_free(void *ptr);

/* BuildRandomVectors, hpc/inverse_power_it.c:12-47: X0[m][p] (vector after
 * vector) = U[0,1) from xoshiro256** seeded with splitmix64(seed). */
int glf_random_vectors(double *X0, unsigned p, unsigned m, uint64_t seed);

/* Synthetic noisy test image of the benchmark configs; not part of
 * the reference. out: height*width bytes. */
int glf_synth_image(uint8_t *out, int width, int height, uint64_t seed);

/* ---- device stages (mirror the hpc/ headers, "glf_" prefixed) -------------------------- */

/* void ComputeAffinityMatrices(Mat* K_A, Mat* K_B, const png_bytep* img, int w, int h,
 *                              unsigned p, const unsigned* idx)   hpc/affinity.h:5, hpc/affinity.c:129-262
 * d_img: device image; sample_indices: HOST array (as in the reference).
 * K_A: dense p x p (allocated here). K_B: KERNEL_B descriptor whose cached
 * degree holds this rank's partial row sums of [K_A K_B] over its pixel rows,
 * already all-reduced when a comm is set. kernel = GLF_KERNEL_*. Pass K_A == NULL
 * to skip materialising K_A. */
int glf_ComputeAffinityMatrices(glf_ctx *ctx, glf_mat *K_A, glf_mat *K_B, const uint8_t *d_img,
                                int width, int height, unsigned sample_size,
                                const unsigned *sample_indices, int kernel, float h_loc, float h_val);

/* void ComputeLaplacianMatrix(Mat* L_A, Mat* L_B, Mat K_A, Mat K_B)  hpc/laplacian.h:3, hpc/laplacian.c:14-42
 * L_A = alpha (diag(D_A) - K_A) dense, L_B = KERNEL_B descriptor with scale -alpha
 * (shares K_B's tables). K_A may be NULL (entries regenerated). alpha_out optional. */
int glf_ComputeLaplacianMatrix(glf_ctx *ctx, glf_mat *L_A, glf_mat *L_B, const glf_mat *K_A,
                               const glf_mat *K_B, double *alpha_out);

typedef struct glf_eig_stats {
    int32_t outer_its, inner_its_total;
    double residual;
    /* the L_A sweeps (block mat-vecs) of the solve: launches, summed device ms (HIP events around the sweep kernel on
     * the context's stream) and the L_A bytes this rank streamed (4 p rows_of_the_rank per sweep) */
    int32_t matvecs;
    float matvec_ms;
    double matvec_bytes;
    int32_t narrow_sweeps;  /* of those sweeps, the ones applied to a packed block of the still-iterating columns only (block PCG) */
    int32_t reserved;
} glf_eig_stats;

/* void InversePowerIteration(const Mat A, unsigned m, Mat* eigvecs, Mat* eigvals,
 *                            PetscBool optiGS, PetscScalar eps)  hpc/inverse_power_it.h:3, hpc/inverse_power_it.c:86-252
 * X0: HOST double [m][p] start block (glf_random_vectors) or NULL for seed 1.
 * eigenvectors: dense p x m (ld = m rounded to 32), the normalised
 * pre-orthogonalisation iterates (:171,:230); eigenvalues: DIAG m = 1/norms (:204).
 * inner_rtol stands in for PETSc's KSP rtol default 1e-5. */
int glf_InversePowerIteration(glf_ctx *ctx, const glf_mat *A, unsigned m, glf_mat *eigenvectors,
                              glf_mat *eigenvalues, int optiGramSchmidt, double epsilon,
                              double inner_rtol, int max_outer, const double *X0,
                              glf_eig_stats *stats);

/* void OrthonormaliseVecs(Vec* X, unsigned n, unsigned p, PetscScalar* norms)  hpc/gram_schmidt.h:4, hpc/gram_schmidt.c:29-64
 * X: dense n x p (row-major, p vectors as columns); norms: HOST double[p] or NULL. */
int glf_OrthonormaliseVecs(glf_ctx *ctx, glf_mat *X, double *norms);
/* void NormaliseVecs(Vec* X, unsigned p, PetscScalar* norms)  hpc/gram_schmidt.h:5 */
int glf_NormaliseVecs(glf_ctx *ctx, glf_mat *X, double *norms);

/* Mat InverseDiagMat(Mat x)  hpc/utils.h (hpc/utils.c:559-586) */
int glf_InverseDiagMat(glf_ctx *ctx, const glf_mat *x, glf_mat *inv);

/* ---- the eigen-solve's operator on its own: one sweep Y = L_A X ---------------------------------------------------------------
 * L_A = alpha (D - K_A) of a KERNEL_B descriptor (L_B of glf_ComputeLaplacianMatrix: scale = -alpha, degree cached), in the form
 * the eigen-solve of the whole path would take under the context's contraction mode and the MV_PATH / PIX_BAND tuning at creation:
 * stored (f32-input MFMA or split-f16 with K slabs, with exact-zero tile skipping when skip_exact_zeros is set and the kernel has a
 * spatial factor), grid-factored, rank form or band form. glf_operator_apply calls the function the block PCG calls, with the same
 * arguments; the decisions of glf_operator_create are the whole-path driver's own (one code). [row0, row1): the rows this operator
 * produces -- 0, p: all of them; otherwise what one rank of the row-sharded solve owns: for a stored L_A (split-f16 contraction
 * only) row0 a multiple of 64 and the column block L_A[:, row0:row1) is what is built; for a factored form whole grid rows (row1 =
 * p closes the last one). ld_hint: the widest ld the caller will apply (the colour, 16-bit and float formats take a factored form
 * only up to ld 64). The descriptor (its image, tables and degree) must outlive the operator.
 * glf_operator_apply: X, Y dense with the same ld, at least p logical rows and round_up(p, 64) rows of storage (what
 * glf_mat_create_dense(round_up(p, 64), ...) gives; the rows from p on of X zero); rows [row0, row1) of Y are written, all ld
 * columns. ld: stored 32, 64, 128 or 256; factored, 8-bit grey: 32 or a multiple of 64 up to 256 (192 included: the widths the
 * block PCG's packed sweeps ask for); factored, other formats: 32 or 64.
 * info (optional) describes the sweep. GLF_ERR_INVALID / GLF_ERR_UNSUPPORTED (a forced MV_PATH that does not apply: not a tensor
 * grid, not the split-f16 contraction, the NLM kernel) name their reason in glf_ctx_last_error and leave Y untouched. */
typedef struct glf_operator glf_operator;
typedef struct glf_operator_info {
    int32_t path;       /* as glf_stats.matvec_path: 0 stored, 1 grid, 3 rank, 4 band */
    int32_t ksplit;     /* stored split-f16 form: K slabs of the last apply; else 0 */
    int32_t skipping;   /* exact-zero skipping in effect */
    int32_t row0, row1;
} glf_operator_info;
int glf_operator_create(glf_ctx *ctx, const glf_mat *L_B, int skip_exact_zeros, unsigned row0, unsigned row1, unsigned ld_hint,
                        glf_operator **op);
int glf_operator_apply(glf_operator *op, const glf_mat *X, glf_mat *Y, glf_operator_info *info);
/* glf_operator_solve: L_A X = B for the first m columns by the eigen-solve's Jacobi-preconditioned block PCG -- the solver's own
 * set-up and loop (one code), with the whole path's preconditioner 1 / (alpha (D_i - 1)) for every form and its per-column rule
 * ||r|| <= rtol ||b||. B, X and R: distinct dense matrices of one ld (32, 64, 128 or 256; the colour, 16-bit and float band forms 32
 * or 64), at least p logical rows and round_up(p, 64) rows of storage; 0 < m <= ld. B is only read. X: the solution; R (or NULL): the
 * PCG's own recurrence residual at exit, not a recomputation of B - L_A X. The padding columns m .. ld - 1 never iterate: X is zero
 * there and R holds B's values; a column of B that is all zero returns X = 0 and costs no step. A solve cut at max_it answers
 * GLF_ERR_NOCONV, and X, R and info then hold the state at the cut. An operator created for a row range is refused
 * (GLF_ERR_UNSUPPORTED: the sharded solve needs a communicator); every refusal names its reason and leaves X and R untouched. The
 * NO_NARROW and OPERAND_MAXIMA tunings act as in the whole path. */
typedef struct glf_solve_info {
    int32_t iters;          /* block PCG steps taken */
    int32_t unconverged;    /* columns still active at exit */
    int32_t matvecs, narrow_sweeps; /* as in glf_eig_stats: timed sweeps (the stored form with f32 operands times none), and the packed ones */
    int32_t path;           /* as glf_operator_info.path */
    int32_t reserved;
} glf_solve_info;
int glf_operator_solve(glf_operator *op, const glf_mat *B, glf_mat *X, glf_mat *R /* or NULL */, unsigned m, double rtol, int max_it,
                       glf_solve_info *info);
/* the stored form's matrix as a dense view (not owned: p rows, row1 - row0 columns, element (k, row) of the symmetric L_A at
 * data[k * ld + row - row0]); GLF_ERR_UNSUPPORTED for a factored form, which stores none */
int glf_operator_stored(const glf_operator *op, glf_mat *view);
int glf_operator_destroy(glf_operator *op); /* NULL: GLF_OK */

/* ---- the PoC's balancing steps of the approximated affinity (inactive experiments in the PoC) ----------
 * sinkhorn(phi, Pi)  python/image_processing.py:90-98: the alternating scalings of K = phi diag(Pi) phi^T, K never formed
 * (200 products K x = phi (Pi o (phi^T x)) for the PoC's 100 iterations). phi: dense N x m in any row order, Pi: diagonal m;
 * d_r, d_c: device double[N]. */
int glf_Sinkhorn(glf_ctx *ctx, const glf_mat *phi, const glf_mat *Pi, int iterations, double *d_r, double *d_c);
/* :99-102: rows [row0, row0 + nrows) of W_AB = diag(r) K diag(c) into d_out (device double [nrows][N]); the PoC keeps the
 * first m rows and splits them into W_A = W_AB[:, :m], W_B = W_AB[:, m:] (:103-104). */
int glf_SinkhornRows(glf_ctx *ctx, const glf_mat *phi, const glf_mat *Pi, const double *d_r, const double *d_c, int64_t row0, int nrows,
                     double *d_out);
/* orthogonalisation(A, B)  :110-127: V = [A ; B^T] A^-1/2 phi_Q Pi_Q^-1/2 with Q = A + A^-1/2 B B^T A^-1/2.
 * d_A: device double n x n (symmetric positive definite), d_B: device double n x q (row-major); d_V: device double
 * (n + q) x n; h_Pi: HOST double[n], clipped at 1. Dense f64 with a one-workgroup Jacobi eigensolver: n <= 512. */
int glf_Orthogonalisation(glf_ctx *ctx, const double *d_A, int n, const double *d_B, int q, double *d_V, double *h_Pi);

/* Mat Nystroem(Mat B, Mat phi_A, Mat Pi_A_Inv, unsigned N, unsigned n, unsigned p)  hpc/nystroem.h:3, hpc/nystroem.c:5-69
 * B: KERNEL_B descriptor (L_B). phi (allocated here): N x m, SAMPLE-FIRST rows:
 * [phi_A ; B^T (phi_A Pi_A_Inv)]. */
int glf_Nystroem(glf_ctx *ctx, const glf_mat *B, const glf_mat *phi_A, const glf_mat *Pi_A_Inv,
                 glf_mat *phi);

/* The same stage with the knobs and the report the whole path has: glf_Nystroem is this call with (0, 0, 0, NULL).
 * skip_exact_zeros: the window of the contraction (glf_options.skip_exact_zeros): the direct kernels pass over the 64-sample chunks,
 *   the grid and rank forms over the k-steps, whose entries are exact zeros of the contraction's arithmetic; same bits, less work.
 *   The colour, 16-bit and float formats' entry-by-entry kernels always run with it.
 * row0 == row1 == 0: all image rows. Otherwise only the image rows [row0, row1) are extended (pixels [row0 width, row1 width): the
 *   geometry one rank of the sharded whole path has); row0 < row1 <= height.
 * phi->data == NULL: phi is allocated here, zero-filled, as glf_Nystroem does. Otherwise phi must be an existing dense N x m
 *   SAMPLE-FIRST matrix of phi_A's ld: the call writes its first p rows (the sample rows, phi_A's bits) and the rows of the
 *   non-sample pixels in the range; every other row keeps its bits.
 * More than 256 eigenpairs (ld a multiple of 256 above 256): all image rows and a phi allocated by the call only; a row range or a
 *   given phi is refused with GLF_ERR_UNSUPPORTED. info then reports the last panel's launch and the entries of all panels.
 * A refusal (bad range, mismatching phi, m > ld) names its reason in glf_ctx_last_error and leaves phi untouched. */
typedef struct glf_nystroem_info {
    int32_t  path;             /* as glf_stats.nystroem_path: 0 direct, 1 grid, 3 rank, 4 band */
    int32_t  contraction;      /* GLF_CONTRACT_* of the kernel that ran */
    int32_t  skipping;         /* 1: the launch ran with a window (SKIP instantiation / skipping passes / band) */
    int32_t  lut;              /* 1: table-driven generation in k_nystroem_f16s */
    uint32_t row0, row1;       /* image rows written */
    double   entries_evaluated;
} glf_nystroem_info;

int glf_Nystroem_ex(glf_ctx *ctx, const glf_mat *B, const glf_mat *phi_A, const glf_mat *Pi_A_Inv,
                    int skip_exact_zeros, unsigned row0, unsigned row1,
                    glf_mat *phi, glf_nystroem_info *info);

/* The degree stage on its own, with the whole path's knobs: D[i] = sum over the image rows [row0, row1) of K(sample i, pixel), this
 * rank's share only (no all-reduce), by the sample tables, coefficients and the degree dispatch glf_ComputeAffinityMatrices and
 * glf_image_processing run. d_img: the guide in the kernel's pixel format; sample_indices: HOST, ascending.
 * skip_exact_zeros: as glf_options.skip_exact_zeros (the grid form's SKIP kernels, the windowed direct sweep); same bits, less work.
 * row0 == row1 == 0: all image rows; otherwise row0 < row1 <= height.
 * h_ysum (optional, HOST [p]): the value-weighted sums U[i] = sum K(sample i, pixel) y[pixel]. Only the grid-factored form has them:
 *   where another form runs the call answers GLF_ERR_UNSUPPORTED and writes nothing.
 * d_plane (optional, device float [height][width]): h_degree receives the joint-filtering sums U_s[i] = sum K(sample i, pixel)
 *   s[pixel] of the grid-factored form instead (operand scale: max |s| over the rows summed); h_ysum must be NULL. Where the grid form
 *   does not apply (not a tensor grid, not an 8-bit grey kernel, DEG_PATH) the call answers GLF_ERR_UNSUPPORTED.
 * info (optional): the caller sets struct_size = sizeof(glf_degree_info); the call fills the rest.
 * A refusal names its reason in glf_ctx_last_error and leaves h_degree, h_ysum and info untouched. */
typedef struct glf_degree_info {
    uint32_t struct_size;
    int32_t  path;        /* 0 dense direct sweep (k_degree), 1 grid-factored, 2 windowed direct (k_degree_win), 5 entry by entry (pixel formats), 6 NLM */
    int32_t  shape;       /* grid only: 0 groups of five m-tiles, 1 one group of ten, 2 window */
    int32_t  skipping;    /* 1: a SKIP / windowed instantiation ran */
    int32_t  chunks;      /* grid: chunks of 512 image rows; direct and entry by entry: chunks of 16 rows */
    int32_t  mgroups;     /* grid only */
    uint32_t row0, row1;  /* image rows summed */
    double   entries_evaluated;
} glf_degree_info;

int glf_Degree_ex(glf_ctx *ctx, const void *d_img, int width, int height, unsigned sample_size, const unsigned *sample_indices,
                  int kernel, float h_loc, float h_val, int skip_exact_zeros, unsigned row0, unsigned row1,
                  const float *d_plane, double *h_degree, double *h_ysum, glf_degree_info *info);

/* Mat Permutation(Mat m, const unsigned* idx, unsigned p)  hpc/utils.h:18, hpc/utils.c:134-173
 * sample-first rows -> raster rows. sample_indices: HOST. */
int glf_Permutation(glf_ctx *ctx, const glf_mat *in, const unsigned *sample_indices,
                    unsigned num_sample_indices, glf_mat *out);

/* png_bytep* ComputeResultFromLaplacian(const png_bytep* img, Mat phi, Mat Pi, unsigned w, unsigned h)
 * hpc/display.h:13, hpc/display.c:58-83 (+ AboveXSetY hpc/utils.c:652, OneColMat2pngbytes :492-534).
 * phi: N x m RASTER rows; Pi: DIAG m (f(eigenvalues)); gain: 3.0 (:73).
 * d_out: device uint8[N]; d_zf: optional device float[N] (z before clamp/cast). */
int glf_ComputeResultFromLaplacian(glf_ctx *ctx, const uint8_t *d_img, const glf_mat *phi,
                                   const glf_mat *Pi, unsigned width, unsigned height, float gain,
                                   uint8_t *d_out, float *d_zf);

/* ---- whole path ----------------------------------------------------------------- */

enum { GLF_FILTER_REFERENCE = 0, GLF_FILTER_POC = 1, GLF_FILTER_SMOOTH = 2, GLF_FILTER_SHARPEN = 3 };
typedef struct glf_options {
    uint32_t struct_size;   /* sizeof(glf_options) */
    uint32_t num_samples;   /* requested sample count; 0 -> width*height*sample_frac (hpc/image_processing.c:187) */
    double sample_frac;     /* 0.01 */
    uint32_t num_eigvals;   /* -num_eigvals; 0 or >= p -> p-1 (hpc/image_processing.c:96-108) */
    int32_t opti_gs;        /* -opti_gs, < 1 -> 1 (:128-140) */
    double epsilon;         /* -inv_it_epsilon, default 0.1 (:142-154) */
    double inner_rtol;      /* 1e-5 (PETSc KSP default) */
    int32_t max_outer;      /* safety cap on outer iterations (reference: none) */
    uint64_t seed;          /* X0 stream */
    float gain;             /* 3.0 hpc/display.c:73 */
    float h_loc, h_val;     /* 40, 30 hpc/affinity.c:117-118 */
    int32_t kernel;         /* GLF_KERNEL_BILATERAL */
    int32_t filter_pow;     /* 1: f(Pi) = Pi (MatPow is a no-op, hpc/utils.c:721); k: Pi^k */
    int32_t filter_mode;    /* GLF_FILTER_REFERENCE (0): z = y + gain Phi Pi^filter_pow Phi^T y, clamp, cast (hpc/display.c:58-83);
                               GLF_FILTER_POC (1): the Python PoC's active filter z = y - Phi diag(mu + 5) Phi^T y
                               (python/image_processing.py:304-305; gain and filter_pow ignored), same clamp and cast;
                               GLF_FILTER_SMOOTH (2): z = Phi diag(1 - mu) Phi^T y -- the PoC's `smoothing` (:197-219), W = I - L with
                               the eigenpairs of the renormalised Laplacian this path computes (W's are (1 - mu, the same vectors);
                               the PoC takes them by a dense eigh of W_A and the same Nystroem extension);
                               GLF_FILTER_SHARPEN (3): z = (1 + beta) W^2 y - beta W^3 y (:222-241) as Phi diag((1 + beta) s^2 -
                               beta s^3) Phi^T y, s = 1 - mu, beta = filter_beta. Neither adds y; gain and filter_pow ignored */
    int32_t skip_exact_zeros; /* 0 (default): every K_B / K_A entry is evaluated, as the reference does.
                                 1: entries that are exactly zero in the arithmetic in use (pixel-sample
                                 distance beyond the radius where exp underflows) are skipped in whole tiles;
                                 the output is bit-identical, the work is not -- see glf_stats.*_evaluated. */
    float filter_beta;      /* GLF_FILTER_SHARPEN: 1.5 (python/image_processing.py:231) */
    int32_t sampling;       /* GLF_SAMPLING_UNIFORM (0): the reference's grid (hpc/sampling.c:6-23); GLF_SAMPLING_RANDOM (1): the PoC's
                               random sampler (python/sampling/random.py:8-16: num_samples distinct pixels, ascending) -- not a tensor
                               grid, so the entry-by-entry kernels and a stored L_A run */
    uint32_t reserved_;
    uint64_t sampling_seed; /* GLF_SAMPLING_RANDOM: seed of the library's own generator (the PoC draws from an unseeded numpy stream) */
} glf_options;
enum { GLF_SAMPLING_UNIFORM = 0, GLF_SAMPLING_RANDOM = 1 };
/* python/sampling/random.py:8-16: *sample_size distinct pixel indices drawn uniformly (xoshiro256** seeded with `seed`), sorted
 * ascending; malloc'd like glf_Sampling's. */
int glf_RandomSampling(int width, int height, unsigned *sample_size, unsigned **sample_indices, uint64_t seed);
void glf_options_default(glf_options *opt);

typedef struct glf_stats {
    uint32_t p, m;
    double alpha;
    glf_eig_stats eig;
    /* device milliseconds (HIP events on the context's stream) */
    float ms_affinity, ms_laplacian, ms_eigen, ms_nystroem, ms_filter, ms_total;
    /* dominant kernel (Nystroem contraction): launches and summed device ms */
    int32_t nystroem_launches;
    float nystroem_kernel_ms;
    int32_t row0, row1;     /* this rank's pixel rows */
    int32_t contraction;    /* GLF_CONTRACT_* actually used */
    int32_t skip_exact_zeros;
    /* kernel entries covered by this rank (dense: p * pixels of the rank), evaluated one by one (direct kernels)
     * or through the factored sums of the grid forms */
    double nystroem_evaluated, degree_evaluated;
    /* f16 MFMA flops issued by the Nystroem contraction (3 products per split multiply-add) */
    double nystroem_mfma_flops;
    int32_t nystroem_path;  /* 0 direct kernel (K_B generated entry by entry), 1 grid-factored (all 256 grey levels),
                               3 grid-factored in rank form (photometric table as a rank-R expansion),
                               4 band form (entry by entry over the samples within the kernel's radius; then nystroem_evaluated
                               counts the entries the kernel evaluated and nystroem_colpass_* describe its launches, with
                               nystroem_colpass_flops = 2 ld x the (pixel, sample) pairs inside the radius). The colour and 16-bit
                               kernels report 0, or 4 with the PIX_BAND tuning key (contraction is then GLF_CONTRACT_F16_SPLIT) */
    int32_t matvec_path;    /* 0 stored L_A streamed per sweep, 1 L_A applied in grid-factored form (never stored), 3 the same in rank form,
                               4 L_A applied in band form (never stored). The colour and 16-bit kernels: 0, or 4 with PIX_BAND */
    /* grid-factored Nystroem: the row-pass kernel (k_grid_rowpass) alone -- launches, summed device ms (HIP events around
     * each launch) and its algorithmic flops 2 rows 256 nc nr ld (one product per multiply-add) */
    int32_t nystroem_rowpass_launches;
    float nystroem_rowpass_ms;
    double nystroem_rowpass_flops;
    /* rank form (nystroem_path 3): the fused T' + column-pass kernel (k_rank_colpass) -- launches, summed device ms (HIP
     * events around each launch), its algorithmic flops 2 ld ncs (sum over rows of (values present) R + pixels) (one product
     * per multiply-add: T' for the (row, value) pairs that occur, then the Ec contraction per pixel), and R, the terms of the
     * expansion of the photometric table (0: exact form) */
    int32_t nystroem_colpass_launches;
    float nystroem_colpass_ms;
    double nystroem_colpass_flops;
    int32_t rank_terms;
    /* 1: the filter ran in the epilogue of the band-form Nystroem kernel (Phi never written; c = Phi^T y from the degree stage's
     * value-weighted sums); ms_filter is then part of ms_nystroem. 0: Phi written, filter as its own stage */
    int32_t filter_fused;
    /* under a communicator: 1 the eigen-solve ran row-sharded (all-gather of the operand per L_A application, all-reduced inner
     * products), 0 every rank ran it on all rows (the default with the band form, whose sweep is cheaper than its all-gather) */
    int32_t eigen_sharded;
    int32_t reserved_;
} glf_stats;

/* ApproximationComputation, hpc/image_processing.c:183-277 (commented tail
 * :240-275 included). d_img: device uint8[height*width], replicated on every
 * rank. d_out: device uint8[height*width]; with a comm of size G rank g fills
 * image rows [g*height/G, (g+1)*height/G) only. d_zf optional float[N].
 * eigvals_out: HOST double[m] or NULL. */
int glf_image_processing(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width,
                         int height, uint8_t *d_out, float *d_zf, double *eigvals_out,
                         glf_stats *stats);

/* Joint filtering: the guide image's graph filter applied to extra signal planes. The graph, the eigenpairs, the filter mode
 * and its weights are those of glf_image_processing on d_img, and d_out / d_zf / eigvals_out / stats are bit-identical to
 * that call's (stats describe the guide). Each plane s_k goes through the same linear operator:
 *   z_k = (1 - ysub) s_k + gain Phi (f(Pi) Phi^T s_k)
 * (reference: s + gain Phi Pi^k Phi^T s; PoC: s - Phi diag(mu + 5) Phi^T s; smooth / sharpen: the same factors as for y).
 * d_sig: device float [nsig][height*width], replicated on every rank like d_img (a depth map, an alpha matte, the chroma of
 * a colour image, ...); d_sig_out: device float [nsig][height*width], not clamped; with a comm rank g writes its own pixel
 * rows only. A plane's result does not depend on the other planes. 1 <= nsig <= GLF_MAX_SIGNALS, else GLF_ERR_INVALID;
 * more than 256 eigenpairs: GLF_ERR_UNSUPPORTED. */
#define GLF_MAX_SIGNALS 4
int glf_image_processing_signals(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width, int height, int nsig,
                                 const float *d_sig, float *d_sig_out, uint8_t *d_out, float *d_zf, double *eigvals_out,
                                 glf_stats *stats);

/* Colour-guided filtering: the graph is built from the RGB differences (GLF_KERNEL_BILATERAL_RGB; opt->kernel must be
 * GLF_KERNEL_BILATERAL or GLF_KERNEL_BILATERAL_RGB, both mean the colour kernel here, any other gives GLF_ERR_UNSUPPORTED) on
 * the sampler of opt->sampling, and each channel x_c of R, G, B goes through the one operator with the filter of
 * opt->filter_mode: z_c = (1 - ysub) x_c + gain Phi f(Pi) Phi^T x_c, then clamped and cast as glf_image_processing's d_out.
 * d_rgb / d_out_rgb: device uint8 [height][width][3] interleaved, d_rgb replicated on every rank; with a comm rank g writes its
 * own pixel rows only. d_zf optional: device float [3][height*width] (planes R, G, B of z before the clamp). eigvals_out: HOST
 * double[m] or NULL. More than 256 eigenpairs: GLF_ERR_UNSUPPORTED. The colour kernel has no grid or rank form: by default the
 * entry-by-entry kernels run and L_A is stored (stats.nystroem_path = matvec_path = 0, filter_fused = 0). With the PIX_BAND tuning
 * key (glf_ctx_set_tuning) the Nystroem stage and the operator take the band form where it applies (nystroem_path / matvec_path 4,
 * L_A not stored, contraction GLF_CONTRACT_F16_SPLIT); the degree and the filter stay entry by entry and unfused. */
int glf_image_processing_rgb(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height, uint8_t *d_out_rgb,
                             float *d_zf, double *eigvals_out, glf_stats *stats);

/* 16-bit greyscale filtering: the graph is built from the 16-bit values (GLF_KERNEL_BILATERAL_U16; opt->kernel must be
 * GLF_KERNEL_BILATERAL or GLF_KERNEL_BILATERAL_U16, both mean the 16-bit kernel here, any other gives GLF_ERR_UNSUPPORTED; opt->h_val
 * is in 16-bit units) on the sampler of opt->sampling, and the image x goes through its filter in the mode of opt->filter_mode:
 * z = (1 - ysub) x + gain Phi f(Pi) Phi^T x, d_out = clamp(x + floor(z - x), 0, 65535) (glf_image_processing's rule at 16 bits).
 * d_img / d_out: device uint16_t [height][width], d_img replicated on every rank; with a comm rank g writes its own pixel rows only.
 * d_zf optional: device float [height*width], z before the clamp. eigvals_out: HOST double[m] or NULL. More than 256 eigenpairs:
 * GLF_ERR_UNSUPPORTED. As for colour the entry-by-entry kernels run and L_A is stored by default (stats.nystroem_path = matvec_path =
 * 0, filter_fused = 0), and the PIX_BAND tuning key selects the band form of the Nystroem stage and the operator. */
int glf_image_processing_u16(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height, uint16_t *d_out,
                             float *d_zf, double *eigvals_out, glf_stats *stats);

/* Joint filtering under a colour or a 16-bit guide: glf_image_processing_signals with the graph of glf_image_processing_rgb /
 * glf_image_processing_u16 (a depth map through a colour image's graph, ...). d_out*, d_zf, eigvals_out and every non-timing field
 * of stats are bit-identical to the plain _rgb / _u16 call's, with or without the PIX_BAND tuning key. d_sig / d_sig_out: device
 * float [nsig][height*width], d_sig replicated on every rank; plane k comes out as z_k = (1 - ysub) s_k + gain Phi (f(Pi) Phi^T s_k),
 * not clamped (sharpening: the Gram-matrix weights, as for the channels); with a comm rank g writes its own pixel rows only. A
 * plane's result does not depend on the other planes. The filter stage reads Phi twice whatever nsig is: once for Phi^T of the
 * channels and the planes together, once for all the outputs. 1 <= nsig <= GLF_MAX_SIGNALS and non-null planes, else
 * GLF_ERR_INVALID; a kernel other than the format's bilateral one, or more than 256 eigenpairs: GLF_ERR_UNSUPPORTED. */
int glf_image_processing_rgb_signals(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, uint8_t *d_out_rgb, float *d_zf, double *eigvals_out,
                                     glf_stats *stats);
int glf_image_processing_u16_signals(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, uint16_t *d_out, float *d_zf, double *eigvals_out,
                                     glf_stats *stats);

/* 32-bit float greyscale filtering: glf_image_processing_u16 on float values (GLF_KERNEL_BILATERAL_F32; opt->kernel must be
 * GLF_KERNEL_BILATERAL or GLF_KERNEL_BILATERAL_F32, both mean the float kernel here, any other gives GLF_ERR_UNSUPPORTED; opt->h_val
 * is in the image's units). d_img / d_out: device float [height][width]; d_out is z = (float)(x + c) with c the f64 correction
 * gain Phi f(Pi) Phi^T x - ysub x: no clamp, no floor, and so no separate float z. The image is checked first, in one pass: a NaN
 * or an Inf anywhere gives GLF_ERR_INVALID (the message names it) and d_out is not written. Routes, tuning keys, declines (more
 * than 256 eigenpairs: GLF_ERR_UNSUPPORTED) and stats as for glf_image_processing_u16. On integer values 0..65535 the graph,
 * the eigenvalues and z have the bits of the 16-bit call's (z: of its d_zf). The _signals call is
 * glf_image_processing_u16_signals under a float guide (the planes are not checked for NaN / Inf); the _capture call writes
 * d_phi_A, d_phi and h_degree. */
int glf_image_processing_f32(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, float *d_out,
                             double *eigvals_out, glf_stats *stats);
int glf_image_processing_f32_signals(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, float *d_out, double *eigvals_out, glf_stats *stats);

/* Float colour filtering: glf_image_processing_rgb on float channels (GLF_KERNEL_BILATERAL_RGBF32; opt->kernel must be
 * GLF_KERNEL_BILATERAL or GLF_KERNEL_BILATERAL_RGBF32, both mean the float colour kernel here, any other gives GLF_ERR_UNSUPPORTED;
 * opt->h_val is in the image's units). d_rgb / d_out_rgb: device float [height][width][3], interleaved; d_out_rgb is z = (float)(x + c)
 * per channel with c the f64 correction: no clamp, no floor, no separate float z. The image's 3 N floats are checked first, in one
 * pass: a NaN or an Inf anywhere gives GLF_ERR_INVALID (the message names it) and d_out_rgb is not written. Routes, tuning keys
 * (PIX_BAND: the band form with three u32 per sample in the chunk tails), declines (the grid / rank / level-table forms, the split-f16
 * direct kernel, the fused filter; more than 256 eigenpairs: GLF_ERR_UNSUPPORTED), stats and eigvals_out as for
 * glf_image_processing_rgb. On integer values 0..255 the graph, the eigenvalues and z
 * have the bits of the 8-bit colour call's (z: of its d_zf, channel by channel). The _signals call is glf_image_processing_rgb_signals
 * under a float colour guide (the planes are not checked for NaN / Inf). */
int glf_image_processing_rgbf32(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height, float *d_out_rgb,
                                double *eigvals_out, glf_stats *stats);
int glf_image_processing_rgbf32_signals(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height, int nsig,
                                        const float *d_sig, float *d_sig_out, float *d_out_rgb, double *eigvals_out, glf_stats *stats);

/* By-products of one glf_image_processing call, for parity checks at sizes where the CPU oracle cannot run the whole
 * path (tests/test_gpu_large.py, bench.py's parity leg): the caller checks sampled rows of Phi / z against
 * hpc/nystroem.c:41-57 and hpc/display.c:58-83 evaluated on the CPU from these. Every pointer is optional. */
typedef struct glf_capture {
    uint32_t struct_size;  /* sizeof(glf_capture) */
    uint32_t ld;           /* out: row stride of phi_A / phi (m rounded up to 32, 64, 128 or 256) */
    float *d_phi_A;        /* device [p rounded up to 64][ld]: the eigenvectors (hpc/inverse_power_it.c:213-241) */
    size_t phi_A_floats;   /* capacity of d_phi_A in floats (GLF_ERR_INVALID when too small) */
    float *d_phi;          /* device [pixels of this rank][ld]: Phi in raster order after Nystroem + Permutation */
    size_t phi_floats;     /* capacity of d_phi in floats */
    double *h_c;           /* host [ld]: right = Phi^T y (hpc/display.c:66), summed over all ranks */
    double *h_degree;      /* host [p]: D_A = rowsum [K_A K_B] (hpc/laplacian.c:18-20), summed over all ranks */
    float *d_corr;         /* device [pixels of this rank]: the correction gain * Phi (f(Pi) Phi^T y) = z - y before it is added to y
                              (hpc/display.c:64-73); the float z resolves it to ulp(z) ~ 4e-6 grey levels only */
    size_t corr_floats;    /* capacity of d_corr in floats */
} glf_capture;
int glf_image_processing_capture(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width, int height,
                                 uint8_t *d_out, float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap);
/* The same by-products of one glf_image_processing_rgb call: d_phi_A, d_phi and h_degree as above; h_c and d_corr are not
 * written (there is one c = Phi^T x_c and one correction per channel: the float z gives them). */
int glf_image_processing_rgb_capture(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height,
                                     uint8_t *d_out_rgb, float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap);
/* The same by-products of one glf_image_processing_u16 call: d_phi_A, d_phi and h_degree; h_c and d_corr are not written (the
 * float z gives the correction). */
int glf_image_processing_u16_capture(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height,
                                     uint16_t *d_out, float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap);

/* The same by-products of one glf_image_processing_f32 call, as for 16 bits. */
int glf_image_processing_f32_capture(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, float *d_out,
                                     double *eigvals_out, glf_stats *stats, glf_capture *cap);

/* The same by-products of one glf_image_processing_rgbf32 call (d_phi_A, d_phi and h_degree), as for 8-bit colour. */
int glf_image_processing_rgbf32_capture(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height,
                                        float *d_out_rgb, double *eigvals_out, glf_stats *stats, glf_capture *cap);

/* ---- the filter stage on its own ---------------------------------------------------------------------------------------------------
 * What turns Phi into pixels, on a Phi the caller gives: c = Phi^T x (the projection), w = f(lam) c (filter_mode, filter_pow,
 * filter_beta and gain as in glf_options, formed as the whole path forms them) and out = rule(x + gain Phi w - ysub x), by the
 * functions the whole path's unfused filter runs. One rank's share: no all-reduce.
 *   pix, d_img, width, height: the guide in the pixel format pix (a GLF_PIX_*), device.
 *   phi: dense N x m, raster rows; ld 32, 64, 128 or 256, or a multiple of 256 above 256 (256-column panels; 8-bit grey guide, no
 *     planes, no sharpening: GLF_ERR_UNSUPPORTED otherwise, as the whole path answers).
 *   lam: HOST [m], the eigenvalues.
 *   row0 == row1 == 0: all image rows; otherwise row0 < row1 <= height, and only the pixels [row0 width, row1 width) are projected
 *     and written (sharpening needs Phi^T Phi over all rows: a proper row range is GLF_ERR_UNSUPPORTED there).
 *   nsig, d_sig, d_sig_out: optional device float planes [nsig][N] in and out, 1 <= nsig <= GLF_MAX_SIGNALS (nsig 0: none).
 *   h_c_in (optional, HOST [channels + nsig][m]): the projection pass is skipped and the weights are formed from it (what a rank
 *     holds after the all-reduce). h_c_out (optional, same shape): the call's own projection over the row range (h_c_in's values
 *     when that is given). h_gram_out (optional, HOST [m][m]): Phi^T Phi, written in sharpening mode only.
 *   d_out: device, the format's output type [N][channels]; d_zf (optional) device float [channels][N]; d_corr (optional, 8-bit grey
 *     guide only, narrow ld) device float [pixels of the range], as glf_capture.d_corr.
 *   info (optional): the caller sets struct_size; the call fills the rest with what ran.
 * A refusal (sample-first phi, bad row range, nsig out of range, m > ld, d_corr with another guide than 8-bit grey, a float guide
 * holding NaN or Inf, ...) names its reason in glf_ctx_last_error and leaves every output untouched.
 * glf_ComputeResultFromLaplacian is this call with lam = Pi, the reference filter, all rows and no planes. */
enum {
    GLF_FK_PHI_T_Y = 1, GLF_FK_PHI_T_SIGNALS = 2, GLF_FK_PHI_T_PIX_SIGNALS = 4, GLF_FK_PHI_GRAM = 8,
    GLF_FK_APPLY = 16, GLF_FK_APPLY_SIGNALS = 32, GLF_FK_APPLY_PIX = 64, GLF_FK_APPLY_PIX_SIGNALS = 128,
    GLF_FK_PLANES = 256, GLF_FK_ACCUM = 512, GLF_FK_FINISH = 1024
};
typedef struct glf_filter_request {
    uint32_t struct_size;   /* sizeof(glf_filter_request) */
    int32_t  pix;
    const void *d_img;
    int32_t  width, height;
    const glf_mat *phi;
    const double *lam;
    int32_t  filter_mode, filter_pow;
    float    filter_beta, gain;
    uint32_t row0, row1;
    int32_t  nsig;
    uint32_t reserved_;
    const float *d_sig;
    float *d_sig_out;
    const double *h_c_in;
    double *h_c_out;
    double *h_gram_out;
    void  *d_out;
    float *d_zf;
    float *d_corr;
} glf_filter_request;
typedef struct glf_filter_info {
    uint32_t struct_size;
    uint32_t kernels;       /* GLF_FK_* bits of the kernels launched */
    uint32_t ld;            /* the LD instantiation of the apply kernel (256 for the panels) */
    uint32_t panels;        /* 256-column panels (0: narrow ld) */
    uint32_t proj_blocks;   /* workgroups of the (last) projection launch, 0 when h_c_in stood in for it */
    uint32_t apply_blocks;  /* workgroups of the (last) apply / accumulate launch */
    uint32_t grid_strided;  /* 1: that launch was capped at 8192 workgroups and strides the rest */
    uint32_t reserved_;
    uint64_t pix0, pix1;    /* the pixels projected and written */
} glf_filter_info;
int glf_Filter_ex(glf_ctx *ctx, const glf_filter_request *rq, glf_filter_info *info);

/* ---- graph handle: build the eigenbasis once, project and synthesize many ------------------------------------------------------
 * Every entry point above builds the graph, solves for the eigenpairs, extends them to every pixel, applies one spectral response
 * and discards everything. The operator is z = ident s + Phi diag(g(mu)) Phi^T s: once Phi exists, any response on any plane is
 * two passes over Phi. A glf_graph keeps Phi (device float [N][ld], raster rows) and the eigenvalues of one image; glf_graph_project
 * forms c = Phi^T s, the caller turns c into coefficients a on the host (glf_filter_coeffs for the library's own four filters, or
 * any response of its own: a band-pass, per-band gains, ...), and glf_graph_synthesize forms ident s + Phi a for up to
 * GLF_GRAPH_MAX_OUTPUTS outputs in one pass over Phi. No reference counterpart (hpc/image_processing.c runs its stages once).
 * Out of scope: contexts that carry a communicator and glf_multi_* (a row-sharded handle: GLF_ERR_UNSUPPORTED); more than 256
 * eigenpairs (GLF_ERR_UNSUPPORTED, the capture calls' own limit); integer or clamped outputs (the outputs are float planes, the
 * caller clamps); a flag of the image_processing host program (it keeps the reference's one-image-in, one-image-out command
 * line); the band-form Nystroem kernel, which is untouched. A graph belongs to its context and is destroyed before it. */
typedef struct glf_graph glf_graph; /* opaque; owns Phi and the eigenvalues */
enum { GLF_PIX_U8 = 0, GLF_PIX_RGB8 = 1, GLF_PIX_U16 = 2, GLF_PIX_F32 = 3, GLF_PIX_RGBF32 = 4 };
#define GLF_GRAPH_MAX_OUTPUTS 32
/* Runs the glf_image_processing*_capture entry point of the pixel format `pix` (d_img in that format, as that entry point takes
 * it) with the handle's Phi as the capture target, allocated as by glf_malloc (not a block of the workspace pool): the graph, the
 * eigenvalues and Phi are bit for bit what that call gives with the same options on the same context, with its routes (PIX_BAND,
 * NYS_PATH, ...), its declines and its refusal of NaN / Inf. opt's filter_mode, gain, filter_pow and filter_beta do not enter the
 * graph. stats: that call's. On any failure *graph is NULL and nothing stays allocated. */
int glf_graph_build(glf_ctx *ctx, const glf_options *opt, int pix, const void *d_img, int width, int height, glf_graph **graph,
                    glf_stats *stats);
int glf_graph_destroy(glf_graph *g); /* NULL: GLF_OK */
typedef struct glf_graph_info {
    uint32_t struct_size;   /* sizeof(glf_graph_info), set by the caller */
    int32_t pix, width, height;
    uint32_t p, m, ld;      /* samples, eigenpairs, row stride of Phi (m rounded up to 32, 64, 128 or 256; columns >= m are zero) */
    const float *d_phi;     /* device [width * height][ld], owned by the handle */
    size_t phi_bytes;
} glf_graph_info;
int glf_graph_get_info(const glf_graph *g, glf_graph_info *info);
int glf_graph_eigenvalues(const glf_graph *g, double *lam /* HOST [m] */);
/* G = Phi^T Phi (the extended eigenvectors are not orthonormal: the sharpening filter needs it); computed on first use, cached */
int glf_graph_gram(glf_graph *g, double *G /* HOST [m][m] */);
/* c_k = Phi^T s_k with f64 sums: one pass over Phi for all planes. 1 <= nplanes <= GLF_MAX_SIGNALS */
int glf_graph_project(glf_graph *g, int nplanes, const float *d_planes /* device [nplanes][N] */, double *h_c /* HOST [nplanes][m] */);
/* out_j = ident[j] * s_{plane[j]} + Phi a_j: one pass over Phi for all outputs (v_mfma_f32_32x32x2_f32: operands (float)a and Phi
 * exactly f32, f32 accumulation in a fixed order; an output's bits do not depend on the outputs beside it). 1 <= nout <=
 * GLF_GRAPH_MAX_OUTPUTS; plane[j] in [0, nplanes) or -1 (no identity term; ident[j] ignored); nplanes may be 0, and ident and
 * d_planes NULL, when every plane[j] is -1. Not clamped. */
int glf_graph_synthesize(glf_graph *g, int nout, const double *h_a /* HOST [nout][m] */, const float *ident, const int *plane,
                         int nplanes, const float *d_planes /* device [nplanes][N] */, float *d_out /* device [nout][N] */);
/* Host only: coefficients a and identity term such that ident * s + Phi a is the library's own filter of opt->filter_mode (opt NULL:
 * the defaults) on a plane whose projection is c. reference: a = gain lam^filter_pow c, ident 1; PoC: a = -(lam + 5) c, ident 1;
 * smooth: a = (1 - lam) c, ident 0; sharpen: a = (1 + beta) L G L c - beta L G L G L c, L = diag(1 - lam), G = gram [m][m], ident 0
 * (gram NULL: GLF_ERR_INVALID). */
int glf_filter_coeffs(const glf_options *opt, unsigned m, const double *lam, const double *gram, const double *c, double *a, float *ident);

/* ---- weighted least-squares fit on a graph handle ----------------------------------------------------------------------------------
 * min_a sum_px w (s - Phi a)^2 + a^T diag(penalty) a has the normal equations (Phi^T diag(w) Phi + diag(penalty)) a = Phi^T diag(w) s:
 * hole filling under a mask, per-pixel confidences, scribble propagation; with w = 1 and no penalty, the orthogonal projection onto
 * the (non-orthonormal) Phi. glf_graph_normal_equations forms both sides in one pass over Phi (k_graph_normal: G on
 * v_mfma_f32_32x32x2_f32 with the pixels as the contraction index, A = fl32(w Phi), B = Phi, f32 chains of at most
 * GLF_GRAPH_NORMAL_CHAIN pixel terms added into f64; b as exact f64 products summed in f64), glf_fit_coeffs solves on the host, and
 * glf_graph_synthesize with no identity term forms the fit Phi a. Summation order and pixel partition depend on (N, ld) alone:
 * two calls give the same bits, G does not depend on nplanes, a plane's b does not depend on the planes beside it. Out of scope:
 * contexts with a communicator (handles refuse them), m > 256. Robust (non-quadratic) data terms: the next section. */
#define GLF_GRAPH_NORMAL_CHAIN 128
/* G = Phi^T diag(w) Phi (HOST [m][m], exactly symmetric) and b_k = Phi^T diag(w) s_k (HOST [nplanes][m]) in one call.
 * d_w: device float [N] or NULL (w = 1). 0 <= nplanes <= GLF_MAX_SIGNALS; with nplanes 0, d_planes and h_b may be NULL.
 * w and the planes are not checked for NaN / Inf or sign. */
int glf_graph_normal_equations(glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_G, double *h_b);
/* Host only: a_k = (G + diag(penalty))^-1 b_k by an f64 Cholesky factorisation, k < nrhs (G's lower triangle is read). penalty NULL = 0.
 * GLF_ERR_INVALID for NULL G / b / a, m = 0, nrhs < 1, or a matrix that is not positive definite
 * (a pivot p with !(p > 0), so NaN is refused too; so is any entry of G or penalty that is not finite); a is then untouched. */
int glf_fit_coeffs(unsigned m, const double *G, const double *penalty, int nrhs, const double *b, double *a);

/* ---- robust fit on a graph handle: iteratively reweighted least squares under Huber, Cauchy and Tukey losses ------------------------
 * The weighted fit is quadratic: the caller has to know which pixels are bad. A robust loss does not ask for that mask:
 * min_a sum_px w rho(q) + the penalty, with q(px) = sum_k ((s_k - Phi a_k)(px) / sigma_k)^2, one weight shared by the 1..4
 * planes (a joint, vector-valued residual: chroma, normals; independent per-plane fits are separate calls). It is solved by IRLS: at
 * the iterate a_prev every pixel gets the weight w_eff = w u(q), u = psi(r) / r, and the next iterate is the weighted fit under w_eff,
 * (G + diag(penalty)) a_k = b_k. The penalty is in the weighted fit's units (with every u = 1 the step is that fit); rho counts a
 * residual in units of sigma_k and halves its square, so the function the iteration decreases (rho is concave in q, d rho / d q =
 * u / 2: majorise-minimise) is F(a) = sum_px w rho(q) + sum_k a_k^T diag(penalty) a_k / (2 sigma_k^2).
 *
 *   loss     u(q)                                      rho(q)
 *   Huber    1 if q <= c^2, else c / sqrt(q)           q / 2 if q <= c^2, else c sqrt(q) - c^2 / 2
 *   Cauchy   1 / (1 + q / c^2)                         (c^2 / 2) log1p(q / c^2)
 *   Tukey    (1 - q / c^2)^2 if q < c^2, else 0        (c^2 / 6) (1 - (1 - min(q / c^2, 1))^3)
 *
 * One iteration's device work (glf_graph_robust_step) is two passes over Phi: k_graph_residual_weight forms d_k = Phi fl32(a_k) on
 * v_mfma_f32_32x32x2_f32 in glf_graph_synthesize's contraction order (d_k has the bits of glf_graph_synthesize's output for the
 * coefficients a_k with no identity term), then in f32 res_k = s_k - d_k, x_k = res_k fl32(1 / sigma_k), q = fmaf(x_k, x_k, q) in
 * ascending k, u by the table with the constants fl32(c), fl32(c^2), fl32(1 / c^2) (Huber: q <= c2 ? 1 : cf / sqrtf(q); Cauchy:
 * 1 / fmaf(q, ic2, 1); Tukey: t = q ic2, t < 1 ? (1 - t)(1 - t) : 0) and w_eff = w u; rho is formed in f64 from (double) q, and loss
 * and mass are per-lane f64 sums added in a fixed order. Then glf_graph_normal_equations' own pass with d_w = w_eff forms G and b: they
 * have the bits of glf_graph_normal_equations(d_weight_out, planes). Two calls give the same bits; a plane's residual plane does not
 * depend on the planes beside it. sigma is the caller's, or the driver's estimate (glf_robust_scale of the plain fit's residuals on a
 * sample of rows); the step never estimates it. Tukey's loss is not convex: the driver starts every loss at the plain weighted fit
 * and does nothing cleverer.
 * Out of scope: per-plane independent weights in one call, a device-side median, L1 / total-variation terms, m > 256, contexts with
 * a communicator and glf_multi_* (handles refuse them), a flag of the image_processing host program; k_graph_normal,
 * k_graph_synthesize, k_graph_cluster and k_graph_transform are untouched. */
enum { GLF_ROBUST_HUBER = 0, GLF_ROBUST_CAUCHY = 1, GLF_ROBUST_TUKEY = 2 };
typedef struct glf_robust_loss {
    uint32_t struct_size;              /* sizeof(glf_robust_loss) */
    int32_t kind;                      /* GLF_ROBUST_* */
    double c;                          /* tuning constant, > 0 and finite; 0 = the 95 % efficiency default: 1.345 / 2.385 / 4.685 */
    double sigma[GLF_MAX_SIGNALS];     /* scale of plane k's residual, > 0 and finite (the step never estimates it) */
} glf_robust_loss;
/* Host only: the f64 statement of the table at q = r^2 >= 0 (c = 0: the default of the kind). u and rho may each be NULL.
 * GLF_ERR_INVALID, u and rho untouched: an unknown kind, a c that is negative or not finite, a q that is negative or NaN. */
int glf_robust_weight(int kind, double c, double q, double *u, double *rho);
/* Host only: sigma = 1.4826 x the median of |res_i| over the entries with w_i > 0 (w NULL: all entries), the median being element
 * floor((cnt - 1) / 2) of the ascending order. GLF_ERR_INVALID, sigma untouched: NULL res / sigma, n = 0, no entry with w > 0, an
 * entry of res or w that is not finite, a median of 0. */
int glf_robust_scale(const double *res, const double *w /* [n] or NULL */, size_t n, double *sigma);
/* One IRLS iteration's device work at the iterate h_a (HOST [nplanes][m]): w_eff = w u(q) of the residuals s_k - Phi a_k,
 * G = Phi^T diag(w_eff) Phi (HOST [m][m]), b_k = Phi^T diag(w_eff) s_k (HOST [nplanes][m]), *h_loss = sum w rho(q) and *h_mass =
 * sum w_eff in f64 (either may be NULL). d_weight_out (device float [N]) receives w_eff and d_res_out (device float [nplanes][N])
 * the residual planes; either may be NULL, and asking for them changes no bit of the rest. 1 <= nplanes <= GLF_MAX_SIGNALS; d_w
 * device float [N] or NULL (w = 1); the planes and w are not checked for NaN / Inf or sign (glf_graph_normal_equations' rule).
 * GLF_ERR_INVALID before any device work, nothing written: a NULL handle / loss / planes / h_a / h_G / h_b, a wrong struct_size, an
 * unknown kind, a c or sigma_k (k < nplanes) that is not finite and positive (c = 0 excepted), an h_a entry that is not finite.
 * Returns with the stream drained. */
int glf_graph_robust_step(glf_graph *g, const glf_robust_loss *loss, const float *d_w, int nplanes, const float *d_planes,
                          const double *h_a, double *h_G, double *h_b, double *h_loss, double *h_mass, float *d_weight_out,
                          float *d_res_out);
typedef struct glf_robust_options {
    uint32_t struct_size;      /* sizeof(glf_robust_options) */
    glf_robust_loss loss;      /* with estimate_sigma set, loss.sigma is not read */
    const double *penalty;     /* HOST [m] or NULL (= 0): fixed over the iterations */
    uint32_t max_iter;         /* 0: 20 */
    double tol;                /* 0: 1e-6 */
    uint32_t sample_rows;      /* rows the scale estimate reads; 0: 4096 */
    int32_t estimate_sigma;    /* 0 | 1 */
} glf_robust_options;
#define GLF_ROBUST_OBJECTIVES 32
typedef struct glf_robust_stats {
    uint32_t struct_size;      /* sizeof(glf_robust_stats), set by the caller */
    uint32_t iterations;       /* steps run */
    int32_t converged;
    double sigma[GLF_MAX_SIGNALS]; /* the scales used (estimated or given); 0 for k >= nplanes */
    double mass;               /* sum w_eff of the last step */
    double objective[GLF_ROBUST_OBJECTIVES]; /* objective[i] = F(a_i) = loss_i + sum_k a_ik^T diag(penalty) a_ik / (2 sigma_k^2) of the
                                                first 32 steps, loss_i the data term the step at its input a_i reports (a_0: the plain
                                                weighted fit); non-increasing up to rounding; the rest 0 */
} glf_robust_stats;
/* The driver. a_0 is the plain weighted fit (glf_graph_normal_equations + glf_fit_coeffs) for every loss. With estimate_sigma: the
 * rows px_i = floor(i N / n_s), n_s = min(sample_rows, N), of Phi, the planes and the weight are gathered, the residuals of a_0
 * formed in f64 on the host and sigma_k = glf_robust_scale of them (a scale of 0, or no sampled pixel of positive weight:
 * GLF_ERR_INVALID, the message says to pass sigma). Then glf_graph_robust_step(a_prev) + glf_fit_coeffs(G, penalty, b) until
 * max |a - a_prev| <= tol max |a| or max_iter steps ran, and optionally one glf_graph_synthesize of the result. h_a HOST
 * [nplanes][m], written; d_fit_out device float [nplanes][N] or NULL; d_weight_out device float [N] or NULL: the last step's
 * weights (those of the last but one iterate); stats or NULL. Refusals before any device work as for glf_graph_robust_step, and
 * a NULL opt, a wrong struct_size (opt's, stats'), an estimate_sigma other than 0 | 1, a tol or penalty entry that is negative or
 * not finite. A system glf_fit_coeffs refuses returns GLF_ERR_INVALID: at a_0 with nothing written, later with h_a, d_fit_out and
 * stats holding the last good iterate. */
int glf_graph_fit_robust(glf_graph *g, const glf_robust_options *opt, const float *d_w, int nplanes, const float *d_planes, double *h_a,
                         float *d_fit_out, float *d_weight_out, glf_robust_stats *stats);

/* ---- spectral segmentation on a graph handle: k-means over the rows of Phi ---------------------------------------------------------
 * The third classic use of the extended eigenvectors: embed every pixel as e(px) = scale o Phi[px][0..dim) (columns in the handle's
 * own order, that of glf_graph_eigenvalues; a 0 in scale drops a column) and cluster the rows (Lloyd's k-means). One iteration is
 * one pass over Phi (k_graph_cluster): the score |c_j|^2 - 2 e . c_j of every pixel against k centroids on v_mfma_f32_32x32x2_f32
 * (operands fl32(scale c_j) and Phi, the fixed contraction order of glf_graph_synthesize: a score's bits do not depend on the
 * centroids beside it), the argmin with the lowest index winning a tie, and in the same pass the per-label sums of the raw rows of
 * Phi (MFMA with the pixels as the contraction index and an exact 0/1 indicator operand, f32 chains of at most GLF_GRAPH_NORMAL_CHAIN
 * pixel terms added into f64), the member counts and the number of labels that moved (exact integers). No atomics; the pixel
 * partition depends on (N, ld) and the device alone: two calls give the same bits. Only the first 32 (ld 32) or 64 (ld >= 64) columns
 * of a row are read, whatever ld is.
 * Unit-length rows and per-pixel weights (the _ex / _w entry points below, the weight and normalise modes of k_graph_cluster):
 * with glf_cluster_embed.normalize the
 * embedding is e(px) = rinv(px) scale o Phi[px][0..dim), rinv = 1 / |scale o Phi[px][0..dim)| formed in f32 in a fixed order (a row
 * of length 0 keeps rinv = 0 and embeds at the origin) -- the row-normalised embedding of Ng, Jordan and Weiss, which is what the
 * Nystroem segmentation paper clusters; without it rinv = 1. A weight plane w (device float [N], NULL = 1; not checked for sign, NaN
 * or Inf: glf_graph_normal_equations' rule) enters the update only: every pixel is labelled, a pixel of weight 0 included, sums_j =
 * sum over the members of j of w rinv Phi[px][c] (raw columns; the caller applies scale), mass_j = sum of w in f64, counts_j and
 * changed count pixels, and the centroid is scale o sums_j / mass_j, a cluster of mass 0 keeping its previous centroid.
 * Out of scope: spherical k-means (renormalised centroids); a margin or confidence output; more than 64 embedding columns;
 * k > GLF_CLUSTER_MAX; contexts with a communicator and glf_multi_* (handles refuse them); a flag of the image_processing host
 * program; k_band, k_graph_synthesize and k_graph_normal, which are untouched. */
#define GLF_CLUSTER_MAX 32
/* One Lloyd iteration. h_cent HOST [k][dim] (embedding space), scale HOST [dim] or NULL (= 1). d_labels device int32 [N], written;
 * d_prev device int32 [N] or NULL, may be d_labels itself (in place). h_sums HOST [k][dim] = the sum of the raw rows of Phi per label
 * (the caller applies scale: glf_cluster_update), h_counts HOST uint64 [k], *changed = the pixels whose label differs from d_prev's
 * (0 without d_prev). GLF_ERR_INVALID before any device work, d_labels untouched: a NULL handle or NULL h_cent / d_labels / h_sums /
 * h_counts / changed, k = 0 or k > GLF_CLUSTER_MAX, dim = 0 or dim > min(m, 64), a centroid or scale entry that is not finite.
 * Returns with the stream drained. */
int glf_graph_cluster_step(glf_graph *g, unsigned k, unsigned dim, const double *h_cent, const double *scale, const int32_t *d_prev,
                           int32_t *d_labels, double *h_sums, uint64_t *h_counts, uint64_t *changed);
/* Host only: cent_j = scale o sums_j / counts_j (scale NULL = 1); an empty cluster keeps cent_prev_j. cent may be cent_prev.
 * GLF_ERR_INVALID, cent untouched: NULL sums / counts / cent, k = 0, dim = 0, an empty cluster without cent_prev. */
int glf_cluster_update(unsigned k, unsigned dim, const double *scale, const double *sums, const uint64_t *counts, const double *cent_prev,
                       double *cent);
/* Host only: k-means++ seeding of k centres among the n rows [n][dim]. It consumes the uniforms u_0 .. u_{k-1} of the stream
 * glf_random_vectors(.., seed) exposes: the first centre is row floor(u_0 n); centre t is the first row, in row order, whose running
 * sum of D^2 exceeds u_t times the total, D^2 the squared distance to the nearest centre chosen so far. GLF_ERR_INVALID, cent
 * untouched: NULL rows / cent, n = 0, dim = 0, k = 0, k > n, or a total that is not positive (fewer than k distinct rows; a NaN). */
int glf_cluster_seed(const double *rows, size_t n, unsigned dim, unsigned k, uint64_t seed, double *cent);
/* The driver. init 0: the rows px_i = floor(i N / n_s), i < n_s = min(sample_rows, N), first dim columns, are gathered to the host,
 * scaled and seeded (glf_cluster_seed with opt->seed); init 1: the caller's h_cent. Then glf_graph_cluster_step + glf_cluster_update
 * with the labels in place, the first step without d_prev, until a step changes no label (converged = 1) or max_iter steps ran. The
 * labels returned are those of the last step, h_cent its update: the usual Lloyd state. max_iter 0 means 50, sample_rows 0 means
 * 4096. One read-back per iteration is the loop's only host poll. Refusals as for glf_graph_cluster_step, and a struct_size that is
 * not sizeof(glf_segment_options), an init other than 0 / 1, or a sample without k distinct rows. */
typedef struct glf_segment_options {
    uint32_t struct_size;  /* sizeof(glf_segment_options), set by the caller */
    uint32_t k, dim;
    uint32_t max_iter;     /* 0: 50 */
    uint32_t sample_rows;  /* 0: 4096 */
    int32_t init;          /* 0: seed from a sample of the rows, 1: the caller's h_cent */
    uint64_t seed;
    const double *scale;   /* HOST [dim] or NULL (= 1) */
} glf_segment_options;
typedef struct glf_segment_stats {
    uint32_t iterations;   /* steps run */
    int32_t converged;
    uint64_t changed_last; /* labels the last step moved (0 when only one step ran) */
    uint64_t counts[GLF_CLUSTER_MAX];
} glf_segment_stats;
int glf_graph_segment(glf_graph *g, const glf_segment_options *opt, int32_t *d_labels, double *h_cent /* HOST [k][dim]: in (init 1) / out */,
                      glf_segment_stats *stats /* or NULL */);
/* The embedding of the _ex calls. NULL, or {normalize 0, d_weight NULL}, is the plain embedding: the call then runs k_graph_cluster
 * itself and every output has the bits of the plain call's. */
typedef struct glf_cluster_embed {
    uint32_t struct_size;   /* sizeof(glf_cluster_embed), set by the caller */
    int32_t normalize;      /* 0 | 1: unit-length rows */
    const float *d_weight;  /* device float [N] or NULL (w = 1) */
} glf_cluster_embed;
/* glf_graph_cluster_step under an embedding. h_sums = sum of w rinv Phi[px][c] per label, h_mass HOST double [k] = sum of w per label
 * (with a plain emb, (double) h_counts), h_counts and *changed count pixels. Refusals as for glf_graph_cluster_step, and an
 * emb->struct_size that is not sizeof(glf_cluster_embed), a normalize other than 0 / 1, a NULL h_mass: all before any device work,
 * d_labels untouched. Two calls give the same bits. */
int glf_graph_cluster_step_ex(glf_graph *g, const glf_cluster_embed *emb, unsigned k, unsigned dim, const double *h_cent, const double *scale,
                              const int32_t *d_prev, int32_t *d_labels, double *h_sums, uint64_t *h_counts, double *h_mass /* HOST [k] */,
                              uint64_t *changed);
/* Host only: cent_j = scale o sums_j / mass_j; a cluster that is empty, !(mass_j > 0), keeps cent_prev_j. Refusals as for
 * glf_cluster_update (NULL sums / mass / cent, k = 0, dim = 0, an empty cluster without cent_prev), cent untouched. */
int glf_cluster_update_w(unsigned k, unsigned dim, const double *scale, const double *sums, const double *mass, const double *cent_prev,
                         double *cent);
/* Host only: k-means++ with probability proportional to w D^2, on the same uniforms as glf_cluster_seed. The first centre is the first
 * row whose running sum of w exceeds u_0 times the total of w; centre t the first row whose running sum of w D^2 exceeds u_t times its
 * total. w HOST [n], or NULL: glf_cluster_seed itself, bit for bit. Refusals as for glf_cluster_seed, and a w that is negative or not
 * finite, or a total (of w, or of w D^2) that is not positive; cent is then untouched. */
int glf_cluster_seed_w(const double *rows, const double *w /* [n] or NULL */, size_t n, unsigned dim, unsigned k, uint64_t seed, double *cent);
/* glf_graph_segment under an embedding; with a plain emb it is glf_graph_segment. Otherwise init 0 gathers the sample rows (and the
 * sample's weights when a plane is given), scales them, normalises them on the host in f64 when asked and seeds with
 * glf_cluster_seed_w; init 1 takes h_cent as it is (embedding space: unit rows when normalize is set). Then glf_graph_cluster_step_ex +
 * glf_cluster_update_w under glf_graph_segment's convergence rule, one read-back per iteration. h_mass: the last step's, or NULL.
 * Refusals as for glf_graph_segment and glf_graph_cluster_step_ex. */
int glf_graph_segment_ex(glf_graph *g, const glf_segment_options *opt, const glf_cluster_embed *emb, int32_t *d_labels, double *h_cent,
                         glf_segment_stats *stats /* or NULL */, double *h_mass /* HOST [k] or NULL */);

/* ---- change of basis on a graph handle: Phi <- Phi T in place, orthonormal Ritz basis -----------------------------------------------
 * The extended eigenvectors are not orthonormal, and the handle's eigenvalues are not sorted. The handle's own data hold the cure,
 * the one-shot orthogonalisation of the Nystroem literature (Fowlkes, Belongie, Chung, Malik) restated on Phi alone: with
 * G = Phi^T Phi = L L^T, Q = Phi L^-T has orthonormal columns and the approximated smoothing operator is W = Phi diag(1 - lam) Phi^T
 * = Q S Q^T, S = L^T diag(1 - lam) L (m x m). With S = U Theta U^T, Phi' = Phi T, T = L^-T U, is an orthonormal eigenbasis of the
 * same W with the eigenvalues lam' = 1 - theta, ascending; W itself does not change. On such a handle Phi^T Phi = I (sharpening
 * needs no Gram matrix), project + synthesize is an orthogonal projector, Graph.fit's smooth penalty is the true energy and "the
 * leading k columns" are the k smoothest.
 * The primitive underneath is glf_graph_transform, Phi <- Phi T for any [m][m_new] matrix (k_graph_transform:
 * v_mfma_f32_32x32x2_f32 with the pixels as the M index, operands Phi and fl32(T) exactly f32, f32 accumulation in
 * glf_graph_synthesize's contraction order, which depends on ld alone; a column's bits depend neither on m_new nor on the other
 * columns of T; a wave reads all ld columns of its 32 rows before it stores the first). It also gives truncation to the leading
 * columns, column reordering and rescaling, and a caller's own rotation (say, the Ritz vectors of a weighted G_w from
 * glf_graph_normal_equations). Out of scope: contexts with a communicator and glf_multi_* (handles refuse them), m > 256, changing
 * ld, a flag of the image_processing host program, Rayleigh-Ritz against the true Laplacian (it needs L Phi over all pixels), a
 * faster glf_graph_gram; k_band, k_graph_synthesize, k_graph_normal and k_graph_cluster* are untouched. A handle that is never
 * transformed gives the bits it gave before. */
/* Phi <- Phi T in place; the handle's m becomes m_new (1 <= m_new <= m), its eigenvalues lam_new, its cached Gram matrix is dropped.
 * h_T HOST [m][m_new] row-major, h_lam_new HOST [m_new]. ld does not change; columns m_new .. ld of Phi become exact zeros. Every
 * later call sees m_new: glf_graph_get_info, _eigenvalues, _project, _synthesize, _normal_equations, _gram (recomputed) and the
 * dim <= min(m, 64) rule of the cluster calls. GLF_ERR_INVALID before any device work, the handle untouched: a NULL argument,
 * m_new = 0 or m_new > m, an entry of T or lam_new that is not finite (or a T entry that does not fit a float). Returns with the
 * stream drained. After a HIP failure inside the call (GLF_ERR_HIP / GLF_ERR_NOMEM) the handle's Phi is unspecified: destroy it. */
int glf_graph_transform(glf_graph *g, unsigned m_new, const double *h_T, const double *h_lam_new);
/* Host only. G [m][m] (lower triangle read). lam NULL: T = L^-T (upper triangular: Gram-Schmidt in column order), lam_new not written.
 * lam [m]: the Ritz basis of Phi diag(1 - lam) Phi^T: T = L^-T U, lam_new = 1 - theta ascending. T [m][m]. f64 Cholesky, then cyclic
 * Jacobi on S; theta descending, the lower original index first on a tie; each column of U signed so that its entry of largest
 * magnitude is positive (the lowest index on a tie). Two calls give the same bits. GLF_ERR_INVALID, T and lam_new untouched: NULL
 * G / T (or lam without lam_new), m = 0, an entry of G or lam that is not finite, a pivot p with !(p > 0). */
int glf_basis_orthonormal(unsigned m, const double *G, const double *lam, double *T, double *lam_new);
enum { GLF_BASIS_CHOLESKY = 0, GLF_BASIS_RITZ = 1 };
typedef struct glf_basis_stats {
    uint32_t struct_size;  /* sizeof(glf_basis_stats), set by the caller */
    uint32_t passes;
    double defect_in;      /* max |Phi^T Phi - I| before the first pass */
    double defect_out;     /* the same after the last pass when verify is set (one more normal-equations pass), else NaN */
} glf_basis_stats;
/* The driver: per pass, G = glf_graph_normal_equations(w NULL, no planes), T = glf_basis_orthonormal (mode RITZ: with the handle's
 * eigenvalues, which become lam_new; mode CHOLESKY: lam NULL, the eigenvalues stay), then glf_graph_transform. A second pass runs in
 * Cholesky mode whatever mode is, so that the Ritz order of the first survives. GLF_ERR_INVALID, the handle untouched: a NULL
 * handle, an unknown mode, passes outside 1..2, a stats->struct_size that is not sizeof(glf_basis_stats), a G that is not positive
 * definite (a later pass that fails leaves the handle as the pass before left it). */
int glf_graph_orthonormalize(glf_graph *g, int mode, int passes /* 1 | 2 */, int verify, glf_basis_stats *stats /* or NULL */);

/* ---- graph handle: project up to 32 planes in one pass over Phi ------------------------------------------------------------------------
 * glf_graph_synthesize writes 32 outputs in one pass over Phi; glf_graph_project and glf_graph_normal_equations take 4 planes, on
 * f64 fma chains that, not the memory, set their time. glf_graph_project_wide is the projection on the matrix pipe
 * (k_graph_project_wide): a 32-channel feature map, the bands of a multispectral cube, a stack of depth hypotheses or the frames of
 * a burst cost one pass instead of ceil(k / 4). Operation by operation: t_k = fl32(w s_k), one f32 multiplication per pixel and
 * plane (d_w NULL: t_k = s_k itself, so NULL and a plane of ones give the same bits); v_mfma_f32_32x32x2_f32 with the pixels as
 * the contraction index, operands t (the 32 plane slots) and Phi exactly as stored (32 columns), every (plane, column) its own f32
 * fma chain over at most GLF_GRAPH_NORMAL_CHAIN pixel terms in ascending pixel order, then added into an f64 image and cleared
 * (k_graph_normal's rule for G); the per-wave and per-workgroup f64 partials are added in a fixed order, no atomics. The pixel
 * partition comes from a fixed per-ld table, so it and the summation order depend on (N, ld) alone: two calls give the same bits; a
 * plane's c depends neither on nplanes, nor on the planes beside it, nor on the slot it sits in; w = 0 gives exact zeros. Against
 * exact arithmetic |c - c*| <= ((GLF_GRAPH_NORMAL_CHAIN + 3) 2^-24 + N 2^-51) sum_px |w s Phi| per entry. Phi is read
 * once at every ld, the planes once (twice at ld 256: the columns are cut into groups of 128). Out of scope: rerouting
 * glf_graph_project, glf_graph_normal_equations or glf_graph_gram through this kernel (their bits stay), contexts with a
 * communicator and glf_multi_* (handles refuse them), m > 256, a flag of the image_processing host program. */
#define GLF_GRAPH_MAX_PLANES 32
/* c_k = Phi^T diag(w) s_k for 1 <= nplanes <= GLF_GRAPH_MAX_PLANES planes in one pass over Phi.
 * d_w: device float [N] or NULL (w = 1); d_planes: device float [nplanes][N]; h_c: HOST double [nplanes][m], m the handle's current
 * m (after glf_graph_transform: m_new). GLF_ERR_INVALID before any device work for a NULL handle, d_planes or h_c, or nplanes
 * outside 1 .. GLF_GRAPH_MAX_PLANES; h_c is untouched on every refusal and every failure. w and the planes are not checked for
 * NaN / Inf or sign (glf_graph_normal_equations' rule): a NaN or Inf in plane k (or in w) reaches c_k (or every c) and no other
 * plane's. Returns with the stream drained. */
int glf_graph_project_wide(glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_c);

/* ---- graph handle: per-pixel quadratic forms (leverage, leave-one-out, distances) ------------------------------------------------------
 * Every other call on a handle returns a linear map of Phi's rows or a reduction over the pixels. glf_graph_quadform returns a
 * quadratic function of one pixel's row, q_k(px) = | R^T phi_px - t_k |^2 with phi_px = Phi[px][0 .. m), for up to
 * GLF_QUAD_MAX_CENTRES centres t_k under one R of up to GLF_QUAD_MAX_COLS columns, in one pass over Phi (k_graph_quadform). With
 * R = L^-T of G_w + diag(penalty) = L L^T (glf_fit_factor) and no centre it is the leverage v = phi^T (G_w + diag(penalty))^-1 phi
 * of the weighted fit: its posterior variance up to the noise variance and, with h = w v, its exact leave-one-out residual
 * e / (1 - h). With R = diag(g) and t_s = g o Phi[seed_s] it is the squared diffusion distance from seed pixels; with a metric R
 * and centroids t_k the squared distances whose softmax (in torch) gives soft memberships.
 * Operation by operation: y_c = sum_j Phi[px][j] fl32(R[j][c]) on v_mfma_f32_32x32x2_f32 in glf_graph_synthesize's contraction
 * order (y_c has the bits of glf_graph_synthesize's output for the coefficient column R[:, c] with no identity term); then in f32,
 * nothing contracted that is not written here: a lane holds 16 columns of each block of 32, the columns c = 32 b + (g & 3) +
 * 8 (g >> 2) + 4 h for g < 16 in half-wave h; per centre q_h = 0, x = y_c - fl32(t_k[c]), q_h = fmaf(x, x, q_h) over b ascending
 * and g ascending; q = q_0 + q_1 (one f32 addition); out_k[px] = q, or out_k[px] + q (one f32 addition) under accumulate.
 * r <= 32 runs one block, r > 32 two: the order depends on that padded column count alone. A column that is zero in R and in every
 * t adds exactly nothing (x = 0), so a plane's bits depend neither on ncent, nor on the centres beside it, nor on appended zero
 * columns; two calls give the same bits; no atomics. Rows past N are neither read nor stored. Against exact arithmetic on the
 * handle's Phi, with x*_c = y*_c - fl32(t_k[c]), delta_c = (ld + 4) 2^-24 sum_j |Phi[px][j] R[j][c]| (glf_graph_synthesize's bound)
 * and eps_c = delta_c + 2^-24 (|x*_c| + delta_c): |q - q*| <= sum_c (2 |x*_c| eps_c + eps_c^2) + (r + 1) 2^-24 sum_c (|x*_c| + eps_c)^2
 * (DESIGN.md). Phi is read once at every ld; the call writes (and under accumulate reads) ncent planes.
 * On a compact handle the column exponents are folded into the rows of R in f64 before the fl32 (R[j][c] 2^e_j, glf_graph_synthesize's
 * rule; t lives in the space of R^T phi and takes no scale): the call returns, bit for bit, what it returns on an f32 handle whose
 * Phi is Q.
 * Out of scope: r > GLF_QUAD_MAX_COLS per launch (the Python wrapper groups, accumulating), per-centre metrics in one call,
 * unit-length rows, soft memberships (a softmax over the output), contexts with a communicator and glf_multi_* (handles refuse
 * them), m > 256, a flag of the image_processing host program. */
#define GLF_QUAD_MAX_COLS 64
#define GLF_QUAD_MAX_CENTRES 32
/* out_k[px] (+)= sum_{c<r} (sum_j Phi[px][j] fl32(R[j][c]) - fl32(t_k[c]))^2, k < ncent.
 * GLF_ERR_INVALID before any device work, d_out untouched: a NULL handle, h_R or d_out, r = 0 or r > GLF_QUAD_MAX_COLS, ncent = 0 or
 * ncent > GLF_QUAD_MAX_CENTRES, an entry of R (after folding) or of t whose fl32 is not finite. accumulate: 0 writes, anything else
 * adds to what d_out holds. Returns with the stream drained. */
int glf_graph_quadform(glf_graph *g, unsigned r, const double *h_R /* HOST [m][r] */, unsigned ncent,
                       const double *h_t /* HOST [ncent][r]; NULL: zeros */, int accumulate, float *d_out /* device [ncent][N] */);
/* Host only: R [m][m] = L^-T of G + diag(penalty) = L L^T (upper triangular), so that phi^T (G + diag(penalty))^-1 phi = |R^T phi|^2.
 * penalty [m] or NULL (zeros). The factorisation and the triangular inverse are glf_basis_orthonormal's. Refusals as glf_fit_coeffs
 * (m = 0, a NULL G or R, not positive definite, NaN, Inf): GLF_ERR_INVALID, R untouched. */
int glf_fit_factor(unsigned m, const double *G, const double *penalty, double *R);
/* h_rows HOST float [nrows][m] <- Phi[h_px[i]][0 .. m) (on a compact handle Q, exact) for 1 <= nrows <= GLF_QUAD_MAX_CENTRES pixel
 * indices 0 <= h_px[i] < N: the rows that become the centres of a distance from seed pixels. The gather is the one behind the seeding
 * of glf_graph_segment. GLF_ERR_INVALID before any device work, h_rows untouched: a NULL argument, nrows outside the range, an index
 * outside the image. Returns with the stream drained. */
int glf_graph_rows(glf_graph *g, unsigned nrows, const int64_t *h_px /* HOST [nrows] */, float *h_rows /* HOST [nrows][m] */);

/* ---- graph handle: compact storage, Phi as f16 with one power-of-two scale per column ---------------------------------------------------
 * The calls on a handle are one or two passes over the resident Phi and run at the memory stream: the only lever left is the number
 * of bytes. glf_graph_compact(g, GLF_PHI_F16) rewrites the handle's Phi as __half [N][ld] (raster rows, the same ld: a row pitch of
 * 2 ld bytes; from glf_malloc, not from the pool) and releases the f32 array; the peak during the call is 1.5 times the f32 size.
 * The quantisation, operation by operation: max_c is the exact maximum of |Phi[px][c]| over the pixels (a maximum: it does not depend
 * on the order); e_c = max(ilogb(max_c), -100) - 14, and e_c = 0 for a column of zeros and for every column >= m; the stored half
 * is f16_rn(Phi[px][c] 2^-e_c): the multiplication is exact, the conversion rounds to nearest even and keeps f16 subnormals. A
 * column's largest stored magnitude therefore lies in [2^14, 2^15] (2^15 when the rounding carries a maximum up to it). The handle then stands for Q[px][c] = 2^e_c half[px][c], with
 * |Q - Phi| <= 2^-11 |Phi| wherever |Phi| >= 2^(e_c - 14) and <= 2^(e_c - 25) below that.
 * The scales never reach the device: the kernels of a compact handle stage the halves through v_cvt_f32_f16 into the LDS image
 * their f32 instances read (csrc/phi_tile.hpp) and keep the MFMA shapes, contraction orders, chain rule and epilogues, and the
 * power-of-two scales, which commute with every rounding the kernels perform, are folded in f64 into the host-side operand before
 * its fl32 (the coefficients a_j[c] 2^e_c of glf_graph_synthesize and of the residuals of glf_graph_robust_step, the scale operand
 * scale_c 2^e_c of the cluster calls) and into the host-side result after its read-back (c_k[c] 2^e_c of glf_graph_project_wide,
 * G[i][j] 2^(e_i + e_j) and b_k[c] 2^e_c of glf_graph_normal_equations and glf_graph_robust_step, sums[j][c] 2^e_c of the cluster
 * steps); the row gathers of the drivers write Q. The contract: on a compact handle every call returns, bit for bit, what it
 * returns on an f32 handle whose Phi is Q, short of under- or overflow of a folded operand in f32. The calls' refusals of operands
 * that are not finite apply to the folded values.
 * A compact handle is taken by glf_graph_synthesize, _project_wide, _normal_equations, _robust_step, _fit_robust, _cluster_step[_ex],
 * _segment[_ex], _eigenvalues, _get_info (d_phi = NULL, phi_bytes = 2 N ld) and _gram (served by the normal-equations pass with
 * w = NULL and cached: a compact handle has no earlier bits to keep). GLF_ERR_UNSUPPORTED, the reason in glf_ctx_last_error and the
 * handle untouched: glf_graph_transform and glf_graph_orthonormalize (compaction is the last step of preparing a handle) and
 * glf_graph_project (its f64-chain kernel reads f32; glf_graph_project_wide is the projection of a compact handle).
 * Out of scope: bf16 or 8-bit storage, compacting during glf_graph_build, a compact handle as input to glf_graph_transform,
 * rerouting glf_graph_project, contexts with a communicator and glf_multi_* (handles refuse them), m > 256, a flag of the
 * image_processing host program, anything inside k_band. */
enum { GLF_PHI_F32 = 0, GLF_PHI_F16 = 1 };
/* storage GLF_PHI_F16: compact the handle as above (on a compact handle: GLF_OK, nothing done). GLF_PHI_F32: GLF_OK and nothing
 * done on an f32 handle, GLF_ERR_UNSUPPORTED on a compact one (there is no way back). GLF_ERR_INVALID, the handle untouched and
 * still f32: a NULL handle (before any device work), another storage value, a max_c (c < m) that is not finite or is >= 2^100.
 * On success the cached Gram matrix is dropped. Returns with the stream drained. */
int glf_graph_compact(glf_graph *g, int storage);
/* *storage (or NULL) <- the format; h_exponent HOST int32 [ld] (or NULL) <- e_c, all 0 on an f32 handle. NULL handle: GLF_ERR_INVALID. */
int glf_graph_storage(const glf_graph *g, int *storage, int32_t *h_exponent /* HOST [ld] or NULL */);
/* d_out device float [N][ld] <- Q (2^e_c half, exact; f32 subnormals kept); on an f32 handle a copy of Phi. GLF_ERR_INVALID for
 * a NULL handle or d_out, before any device work. Returns with the stream drained. */
int glf_graph_dequantize(glf_graph *g, float *d_out /* device [N][ld] */);

/* ---- graph handle: the spectral edge map, neighbour differences of Phi ------------------------------------------------------------------
 * Every other call on a handle treats the rows of Phi as an unordered set. glf_graph_edges uses that they lie on the image raster:
 * for the neighbours nb of a pixel px = (row, col) -- E (row, col + 1), S (row + 1, col), SE (row + 1, col + 1), SW (row + 1, col - 1)
 * -- it returns out(px) = sum_{c < dim} (scale_c (Phi[nb][c] - Phi[px][c]))^2, the squared distance in the embedding between the two
 * pixels (k_graph_edges, the handle's stencil kernel). With scale = g(lam) it is the boundary signal sum_c g_c^2 (v_c(px) - v_c(nb))^2
 * of normalised-cuts contour detection, and the edge weights of the 4- / 8-connected pixel graph in the spectral metric that a
 * watershed, a random walker or an edge-stopping function consume; glf_graph_quadform with seed centres is its global counterpart.
 * The sample pixels' rows of Phi are phi_A's own bits, every other row is extended, and the two differ in scale (README, "Spectral
 * edge map"): an edge that touches a sample pixel is an outlier. Hence the validity mask, and glf_graph_samples, which says where
 * the samples are.
 * Planes: plane k belongs to the k-th set bit of dirs in ascending order, [popcount(dirs)][N] floats. A plane's value is +0 (the bit
 * pattern) where nb lies outside the image, or d_valid is given and valid[px] or valid[nb] is 0: E and SE at col = W - 1, SW at
 * col = 0, S / SE / SW on the last row. The raster neighbour px + 1 of the next image row is never taken for E. Every pixel of every
 * requested plane is written, nothing else is.
 * Operation by operation, in f32, nothing contracted that is not written here: s_c = fl32(scale_c); q = +0; for c = 0 .. dim - 1
 * ascending, one chain per (pixel, direction): d = Phi[nb][c] - Phi[px][c] (one subtraction), x = s_c d (one multiplication),
 * q = fmaf(x, x, q). The chain continues across the staged column chunks (CW = min(ld, 64); a partial sum that is stored and
 * reloaded between chunks keeps its bits). A plane's bits therefore depend neither on dirs, nor on ld, nor on the launch geometry,
 * nor on d_valid where the edge is live; a column with scale 0 changes nothing (x = +-0, fmaf(x, x, q) = q); two calls give the same
 * bits; no atomics. Columns at or beyond dim rounded up to CW are not read (the cluster step's rule); the columns between dim and
 * that bound are read and multiplied by 0, so they must be finite (columns >= m are zeros).
 * Against exact arithmetic on the handle's Phi with the scale fl32(scale), q* = sum_c (s_c (Phi[nb][c] - Phi[px][c]))^2:
 * |q - q*| <= gamma(dim + 4) q* + dim 2^-149, gamma(n) = n 2^-24 / (1 - n 2^-24) ("Spectral edge map").
 * On a compact handle 2^e_c is folded into scale_c in f64 before its fl32 (the cluster calls' rule): the call returns, bit for bit,
 * what it returns on an f32 handle whose Phi is Q (glf_graph_dequantize), short of under- or overflow of a folded scale in f32.
 * Out of scope: a full (non-diagonal) metric, unit-length rows, Gaussian-derivative or oriented filters wider than one pixel,
 * non-maximum suppression, watershed, connected components, repairing the scale of Phi's sample rows, contexts with a communicator
 * and glf_multi_* (handles refuse them), m > 256, a flag of the image_processing host program. */
enum { GLF_EDGE_E = 1, GLF_EDGE_S = 2, GLF_EDGE_SE = 4, GLF_EDGE_SW = 8 };   /* neighbour (row, col+1), (row+1, col), (row+1, col+1), (row+1, col-1) */
/* GLF_ERR_INVALID before any device work, d_out untouched, the reason in glf_ctx_last_error: dirs 0 or above 15, dim 0 or above m, a
 * scale (after folding) whose fl32 is not finite, a NULL d_out; a NULL handle likewise (there is no context to take the reason).
 * d_valid is not checked. Returns with the stream drained. */
int glf_graph_edges(glf_graph *g, unsigned dirs, unsigned dim, const double *h_scale /* HOST [dim] or NULL = ones */,
                    const uint8_t *d_valid /* device [N] or NULL */, float *d_out /* device [popcount(dirs)][N] */);
/* h_idx HOST [p] <- the sample pixels of the build call, ascending pixel indices: the list of glf_graph_build's own sampler call
 * (glf_Sampling or glf_RandomSampling under the build's options), kept in the handle; p is glf_graph_info.p. GLF_ERR_INVALID for a NULL handle, and for a NULL h_idx with the reason
 * in glf_ctx_last_error. */
int glf_graph_samples(const glf_graph *g, unsigned *h_idx /* HOST [p], ascending pixel indices */);

/* ---- graph handle: label read-out, the per-pixel winner of up to 32 score planes and its margin -----------------------------------------
 * Supervised labelling on a handle -- scribbles propagated to every pixel, a network's class logits smoothed through the graph, a
 * stack of depth hypotheses resolved per pixel -- ends in one step: form the k score planes ident_j s_j + Phi a_j and take, per
 * pixel, the winner and how clearly it won. glf_graph_classify forms the scores in registers in one pass over Phi
 * (k_graph_classify: glf_graph_synthesize's kernel up to its store) and writes up to three planes, the label, the best score and
 * the margin, instead of the k score planes a caller would write with glf_graph_synthesize and read back for an argmax.
 * Scores, operation by operation. h_a, ident, plane, nplanes and d_planes mean what they mean in glf_graph_synthesize: acc_j =
 * sum_c Phi[px][c] fl32(a_j[c]) on v_mfma_f32_32x32x2_f32 in its contraction order; z_j = fmaf(ident[j], planes[plane[j]][px], acc_j)
 * where plane[j] >= 0 and z_j = acc_j otherwise. With h_bias = NULL score_j = z_j has the bits of glf_graph_synthesize's output j;
 * with a bias score_j = z_j + fl32(bias_j), one f32 addition (a bias of zeros therefore turns a score of -0 into +0 and changes
 * nothing else).
 * Read-out, in f32, nothing contracted that is not written here. Comparisons are IEEE: a NaN compares false, +0 and -0 are equal.
 *   best  = max_j score_j under a strict >, from -inf with label 0: b = -inf, l = 0; for j = 0 .. k - 1 ascending: if score_j > b
 *           then b = score_j, l = j. A NaN score never wins; of equal scores the lowest j wins (+0 and -0 tie, and best keeps the
 *           sign of the winner's); a pixel with no score above -inf gets label 0 and best -inf.
 *   label = l, the lowest j < k with score_j == best where there is one.
 *   second = the same maximum over j != label, from -inf.
 *   margin = +0 where second == best (a tie, two infinities of one sign, and best = -inf: never a NaN and never -0), else
 *           best - second, one f32 subtraction: +inf for k = 1 and wherever second is -inf and best is not.
 * How the kernel gets there: a lane holds the 16 scores j = (g & 3) + 8 (g >> 2) + 4 h, g < 16, of its pixel in half-wave h and
 * runs the top two over g ascending (s > b: second = b, b = s, l = j; else s > second: second = s); one exchange with the other
 * half-wave; the other half wins if b' > b or (b' == b and l' < l); second = max(min(b, b'), max(second, second')). The slots
 * j >= k are masked by index: whatever they hold, they change nothing. The result is the sequential rule above for every input,
 * NaN and infinities included (tests/test_classify_ref.py restates both and compares them).
 * A class takes part in the same way in every slot; only the tie rule sees the order. Two calls give the same bits; no atomics;
 * rows past N are neither read nor stored; an output whose pointer is NULL is not written, every pixel of the others is. Phi is
 * read once at every ld, the identity planes once per class that names them (where any class has an identity term, a class
 * without one reads plane 0's pixel and drops it: the loads are unconditional so that they are all in flight together).
 * On a compact handle 2^e_c is folded into a_j[c] in f64 before its fl32 (glf_graph_synthesize's rule), so the scores are that
 * handle's own synthesize outputs bit for bit, and the call returns what it returns on an f32 handle whose Phi is Q.
 * Out of scope: per-class counts, k > GLF_CLASSIFY_MAX and merging across groups, a label input to the projection, contexts with
 * a communicator and glf_multi_* (handles refuse them), m > 256, a flag of the image_processing host program. (Softmax
 * confidences and mean-field iterations: glf_graph_softmax below.) */
#define GLF_CLASSIFY_MAX 32   /* = GLF_GRAPH_MAX_OUTPUTS */
/* GLF_ERR_INVALID before any device work, every output untouched, the reason in glf_ctx_last_error: k outside 1 ..
 * GLF_CLASSIFY_MAX, a NULL h_a or plane, nplanes < 0, a plane[j] outside -1 .. nplanes - 1, an identity term with a NULL ident or
 * d_planes, all three output pointers NULL, a coefficient (after folding) or a bias whose fl32 is not finite; a NULL handle
 * likewise (there is no context to take the reason). The planes are not checked. Returns with the stream drained. */
int glf_graph_classify(glf_graph *g, int k, const double *h_a /* HOST [k][m] */, const float *ident /* HOST [k] */,
                       const int *plane /* HOST [k] */, int nplanes, const float *d_planes /* device [nplanes][N] */,
                       const double *h_bias /* HOST [k] or NULL */, int32_t *d_label /* device [N] or NULL */,
                       float *d_best /* device [N] or NULL */, float *d_margin /* device [N] or NULL */);

/* ---- graph handle: softmax read-out, class probabilities, log-sum-exp and entropy of up to 32 score planes ---------------------------
 * Where glf_graph_classify returns the winner, glf_graph_softmax returns how the k classes share a pixel: p_j = exp(beta score_j) /
 * sum_i exp(beta score_i), the log-sum-exp lse = log sum_j exp(beta score_j) and the entropy -sum_j p_j ln p_j. Per-pixel class
 * probabilities of graph-smoothed logits, an uncertainty map, the soft memberships of a set of centres and one mean-field step of a
 * dense CRF end in this call. The scores are formed in registers in one pass over Phi (k_graph_softmax: k_graph_classify up to its
 * scores) instead of being written by glf_graph_synthesize, read and rewritten by a softmax and read again for the entropy.
 * Scores. h_a, ident, plane, nplanes, d_planes and h_bias mean what they mean in glf_graph_classify, and score_j is
 * glf_graph_classify's score_j bit for bit: acc_j on v_mfma_f32_32x32x2_f32 in glf_graph_synthesize's contraction order, z_j =
 * fmaf(ident[j], planes[plane[j]][px], acc_j) where plane[j] >= 0 and acc_j otherwise, then one f32 addition of fl32(bias_j) when
 * h_bias is given. The scores are those of j < k: the slots j >= k are masked by index and never enter.
 * Read-out, in f32, nothing contracted that is not written here. A lane holds the 16 scores j = (g & 3) + 8 (g >> 2) + 4 h, g < 16,
 * of its pixel in half-wave h; "per lane" below runs over the lane's classes < k with g ascending, and "exchange" is one
 * __shfl_xor(.., 32) with the lane that holds the pixel's other 16 classes.
 *   best   b = -inf; per lane: if score_j > b then b = score_j; exchange: if b' > b then b = b'. (glf_graph_classify's best: a NaN
 *          never enters.)
 *   t_j    d_j = score_j - best (one subtraction); t_j = beta2 * d_j (one multiplication), beta2 = fl32(beta log2 e), the product
 *          formed in f64 on the host.
 *   e_j    v_exp_f32(t_j) (2^t at 1 ulp; a result below 2^-126 is flushed to +0).
 *   S      per lane from +0: S = S + e_j; exchange: S = S + S'. (Both halves hold the same bits.)
 *   A      per lane from +0: A = fmaf(e_j, e_j > 0 ? t_j : 0, A); exchange: A = A + A'. (sum_j e_j t_j with 0 * -inf read as 0: a
 *          class at -inf, or flushed to e_j = +0, adds +0 or -0 and changes no bit. Formed only where d_entropy is given.)
 *   p_j    r = 1 / S, one correctly rounded f32 division; p_j = e_j * r. Plane j of d_prob gets p_j.
 *   lse    fmaf(fl32(ln 2), L, fl32(beta) * best), L = v_log_f32(S).
 *   entropy  fl32(ln 2) * (L - A * r): one multiplication, one subtraction, one multiplication.
 * Special values follow from these operations: a score of -inf beside a finite one gives e_j = p_j = +0 exactly; a pixel with a
 * NaN score, a +inf score or nothing but -inf scores has S = NaN and every requested output NaN (all k probabilities, lse and
 * entropy); no other pixel is affected. k = 1 gives p = 1, entropy +0 and lse = fl32(beta) * score (+ (+0)).
 * Scaling the scores by a power of two and beta by its inverse changes no bit of p and entropy, short of under- and overflow.
 * Error against the exact softmax of the same f32 scores, u = 2^-24, t*_j = beta log2 e (score_j - best) ("Softmax
 * read-out"): eps_j = 2 u + 3 ln 2 |t*_j| u, eps_S = max over the classes with t*_i >= -126 of eps_i + 16 u;
 * |p_j - p*_j| <= p*_j (eps_j + eps_S + 3 u) (1 + 2^-10) + 2^-126; lse and entropy: DESIGN.md.
 * Two calls give the same bits; no atomics; rows past N are neither read nor stored; an output whose pointer is NULL is neither
 * computed nor written, every pixel of the others is, and asking for fewer outputs changes no bit of the ones asked for. d_prob
 * must not overlap d_planes (stated, not detected). Phi is read once at every ld, the identity planes as in glf_graph_classify.
 * On a compact handle 2^e_c is folded into a_j[c] in f64 before its fl32 (glf_graph_synthesize's rule): the call returns what it
 * returns on an f32 handle whose Phi is Q. There is no new host-only function, hence no make ..._check target.
 * Out of scope: k > GLF_SOFTMAX_MAX and merging across groups, unit-length rows in soft memberships, subtracting the self-message
 * of a mean-field step, a C driver for mean field (Graph.mean_field in glf.py drives glf_graph_project_wide and this call), fusing
 * the re-projection of p into this pass, repairing the scale of Phi's sample rows, contexts with a communicator and glf_multi_*
 * (handles refuse them), m > 256, a flag of the image_processing host program. */
#define GLF_SOFTMAX_MAX 32   /* = GLF_GRAPH_MAX_OUTPUTS */
/* GLF_ERR_INVALID before any device work, every output untouched, the reason in glf_ctx_last_error: everything
 * glf_graph_classify refuses (k outside 1 .. GLF_SOFTMAX_MAX, a NULL h_a or plane, nplanes < 0, a plane[j] outside -1 ..
 * nplanes - 1, an identity term with a NULL ident or d_planes, a coefficient (after folding) or a bias whose fl32 is not finite),
 * all three output pointers NULL, a beta whose fl32 is not finite and positive or whose beta log2 e is not finite in f32; a NULL
 * handle likewise (there is no context to take the reason). The planes are not checked. Returns with the stream drained. */
int glf_graph_softmax(glf_graph *g, int k, const double *h_a /* HOST [k][m] */, const float *ident /* HOST [k] */,
                      const int *plane /* HOST [k], -1: none */, int nplanes, const float *d_planes /* device [nplanes][N] */,
                      const double *h_bias /* HOST [k] or NULL */, double beta, float *d_prob /* device [k][N] or NULL */,
                      float *d_lse /* device [N] or NULL */, float *d_entropy /* device [N] or NULL */);

/* ---- graph handle: blend read-out, a bank of up to 32 score planes read out per pixel by a level map -----------------------------------
 * Every filtering call on a handle applies one response to the whole image. "Denoise more here than there" -- a sensor's noise-level
 * map, a brush mask, depth-dependent blur, foveation, a confidence map -- needs a strength per pixel, and rendering per-segment models
 * a_j needs out(px) = Phi[px] . a_label(px). Both are one operation: form a small bank of score planes z_b = ident_b s + Phi a_b and
 * read out, per pixel, the plane that a map selects, or the linear blend of its two neighbours. glf_graph_blend forms the bank in
 * registers in one pass over Phi (k_graph_blend: k_graph_classify up to its scores) and writes the nout read-outs, instead of the
 * nout * nlevels planes a caller would write with glf_graph_synthesize and read back for a gather and a lerp.
 * Slots. The bank holds nout outputs of nlevels levels each, slot s = o * nlevels + b, nout * nlevels <= GLF_BLEND_MAX_SLOTS; one level
 * map d_level serves all outputs of a call. h_a, ident, plane, nplanes and d_planes mean per slot what they mean per output in
 * glf_graph_synthesize: acc_s = sum_c Phi[px][c] fl32(a_s[c]) on v_mfma_f32_32x32x2_f32 in its contraction order, with
 * glf_graph_synthesize's bits for coefficient row s.
 * Read-out per pixel px, in f32, nothing contracted that is not written here:
 *   t   = d_level[px]
 *   tc  = fminf(fmaxf(t, 0), (float)(nlevels - 1))      a NaN level reads as level 0; -inf and +inf clamp to the two ends
 *   i   = min((int)tc, nlevels - 2)                     (truncation)
 *   f   = tc - (float)i                                 exact (Sterbenz); 0 <= f <= 1, and f = 1 only at tc = nlevels - 1
 *   for output o: lo = o * nlevels + i, hi = lo + 1
 *   z_s = plane[s] >= 0 ? fmaf(ident[s], planes[plane[s]][px], acc_s) : acc_s    for s in {lo, hi} only: glf_graph_synthesize's
 *         output for slot s, bit for bit
 *   out_o[px] = f == 0 ? z_lo : f == 1 ? z_hi : fmaf(f, z_hi, fmaf(-f, z_lo, z_lo))
 * The two scores are chosen by their index (selects), never by arithmetic over the bank: a slot that a pixel does not take with a
 * weight other than zero cannot reach that pixel's output, whatever it holds (NaN, Inf) -- at an integer level the output is the
 * level's plane bit for bit, and levels appended above the map's maximum change no bit. An output depends neither on nout nor on the
 * outputs beside it. How the kernel gets there: a lane holds the 16 slots (g & 3) + 8 (g >> 2) + 4 h, g < 16, of its pixel in
 * half-wave h (slot s lives in half (s >> 2) & 1); the wave writes its accumulators to its own LDS image as [pixel][slot] and every
 * read-out is two indexed reads of the pixel's row (tests/blend_ref.py restates the ownership, the index rule and the lerp).
 * Error against exact arithmetic on the handle's own Phi with the same f32 level (hence the same i and f), u = 2^-24 (DESIGN.md,
 * "Blend read-out"): |out - out*| <= (1 - f) e_lo + f e_hi + 2 u (1 + u) ((1 - f) (|z*_lo| + e_lo) + f (|z*_hi| + e_hi)), e_s =
 * (ld + 4) u (|ident_s s| + |Phi| |a_s|) being glf_graph_synthesize's bound, short of underflow.
 * Two calls give the same bits; no atomics; rows past N are neither read nor stored, d_level[px] is read for px < N only; every
 * pixel of the nout planes of d_out is written. d_out must not overlap d_planes or d_level (stated, not detected). Phi is read once
 * at every ld, the level map once, and where any slot has an identity term two plane values per output and pixel (a slot without a
 * term reads plane 0's pixel and drops it).
 * On a compact handle 2^e_c is folded into a_s[c] in f64 before its fl32 (glf_graph_synthesize's rule): the call returns what it
 * returns on an f32 handle whose Phi is Q. There is no new host-only function, hence no make ..._check target.
 * Out of scope: per-output level maps, more than GLF_BLEND_MAX_SLOTS slots per launch (Graph.blend in glf.py groups by outputs),
 * non-linear interpolation between levels, a derivative with respect to the level, evaluating a response per pixel and column
 * instead of a bank, general per-pixel mixture weights over all levels, an int32 label input (Graph.gather converts), a C driver for
 * a piecewise fit (Graph.fit_piecewise drives glf_graph_normal_equations and this call), contexts with a communicator and
 * glf_multi_* (handles refuse them), m > 256, a flag of the image_processing host program. */
#define GLF_BLEND_MAX_SLOTS 32   /* = GLF_GRAPH_MAX_OUTPUTS */
/* GLF_ERR_INVALID before any device work, d_out untouched, the reason in glf_ctx_last_error: nout < 1, nlevels < 2 or nout * nlevels >
 * GLF_BLEND_MAX_SLOTS, a NULL h_a or plane, nplanes < 0, a NULL d_level or d_out, a plane[s] outside -1 .. nplanes - 1, an identity
 * term with a NULL ident or d_planes, a coefficient (after folding) whose fl32 is not finite; a NULL handle likewise (there is no
 * context to take the reason). The planes and the level map are not checked. Returns with the stream drained. */
int glf_graph_blend(glf_graph *g, int nout, int nlevels, const double *h_a /* HOST [nout * nlevels][m], slot = o * nlevels + b */,
                    const float *ident /* HOST [nout * nlevels] or NULL */, const int *plane /* HOST [nout * nlevels], -1: none */,
                    int nplanes, const float *d_planes /* device [nplanes][N] or NULL */, const float *d_level /* device [N] */,
                    float *d_out /* device [nout][N] */);

/* Throughput mode for a batch of equally sized tiles (BASELINE.json configs[4]: "batch of 64 x 1024x1024 noisy tiles
 * sharing one sample set"; hpc/sampling.c:6-23 gives tiles of one size the same sample grid). The reference would run its
 * main once per tile (hpc/image_processing.c:279-335); here tile t = d_imgs + t*width*height goes through
 * glf_image_processing unchanged on one of `nctx` contexts (one stream + one host thread each, tiles dealt dynamically),
 * so every output is bit-identical to the single-image call's. Replicas only: the contexts must not carry a comm.
 * d_outs: uint8[ntiles*height*width]; d_zfs (optional) float[ntiles*N]; stats (optional) HOST glf_stats[ntiles].
 * On failure returns the first failing tile's status; the message is in ctxs[0]'s last error. */
int glf_image_processing_batch(glf_ctx *const *ctxs, int nctx, const glf_options *opt, const uint8_t *d_imgs,
                               int width, int height, int ntiles, uint8_t *d_outs, float *d_zfs, glf_stats *stats);

/* ReadAndBcastImage + ApproximationComputation + the gather of the result (hpc/image_processing.c:45-76, 183-277,
 * hpc/utils.c:502-527): h_img / h_out are HOST buffers of height*width bytes; every rank receives the whole image, runs
 * glf_image_processing on its pixel rows and writes them into h_out (h_zf optional float[N]). stats: HOST glf_stats[n]
 * or NULL; eigvals_out: HOST double[m] or NULL (rank 0's, identical on every rank). */
int glf_multi_image_processing(glf_multi *w, const glf_options *opt, const uint8_t *h_img, int width, int height,
                               uint8_t *h_out, float *h_zf, double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing with signal planes (glf_image_processing_signals): h_sig HOST float [nsig][height*width] goes
 * to every rank whole; each rank's pixel rows of the filtered planes are gathered into h_sig_out (HOST float
 * [nsig][height*width]). */
int glf_multi_image_processing_signals(glf_multi *w, const glf_options *opt, const uint8_t *h_img, int width, int height,
                                       int nsig, const float *h_sig, float *h_sig_out, uint8_t *h_out, float *h_zf,
                                       double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing for colour (glf_image_processing_rgb): h_rgb / h_out_rgb HOST uint8 [height][width][3]; each rank's
 * pixel rows are gathered into h_out_rgb (h_zf optional HOST float [3][height*width]). */
int glf_multi_image_processing_rgb(glf_multi *w, const glf_options *opt, const uint8_t *h_rgb, int width, int height,
                                   uint8_t *h_out_rgb, float *h_zf, double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing for 16-bit grey (glf_image_processing_u16): h_img / h_out HOST uint16_t [height][width]; each rank's
 * pixel rows are gathered into h_out (h_zf optional HOST float [height*width]). */
int glf_multi_image_processing_u16(glf_multi *w, const glf_options *opt, const uint16_t *h_img, int width, int height,
                                   uint16_t *h_out, float *h_zf, double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing_rgb / _u16 with signal planes (glf_image_processing_rgb_signals / _u16_signals): h_sig and h_sig_out
 * HOST float [nsig][height*width] as for glf_multi_image_processing_signals. */
int glf_multi_image_processing_rgb_signals(glf_multi *w, const glf_options *opt, const uint8_t *h_rgb, int width, int height,
                                           int nsig, const float *h_sig, float *h_sig_out, uint8_t *h_out_rgb, float *h_zf,
                                           double *eigvals_out, glf_stats *stats);
int glf_multi_image_processing_u16_signals(glf_multi *w, const glf_options *opt, const uint16_t *h_img, int width, int height,
                                           int nsig, const float *h_sig, float *h_sig_out, uint16_t *h_out, float *h_zf,
                                           double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing for float grey (glf_image_processing_f32 / _f32_signals): h_img / h_out HOST float [height][width]. The
 * NaN / Inf check runs on the host image before any rank starts: a refused image leaves the world usable. */
int glf_multi_image_processing_f32(glf_multi *w, const glf_options *opt, const float *h_img, int width, int height, float *h_out,
                                   double *eigvals_out, glf_stats *stats);
int glf_multi_image_processing_f32_signals(glf_multi *w, const glf_options *opt, const float *h_img, int width, int height, int nsig,
                                           const float *h_sig, float *h_sig_out, float *h_out, double *eigvals_out, glf_stats *stats);

/* glf_multi_image_processing for float colour (glf_image_processing_rgbf32 / _rgbf32_signals): h_rgb / h_out_rgb HOST float
 * [height][width][3]. The NaN / Inf check runs on the host image before any rank starts: a refused image leaves the world usable. */
int glf_multi_image_processing_rgbf32(glf_multi *w, const glf_options *opt, const float *h_rgb, int width, int height, float *h_out_rgb,
                                      double *eigvals_out, glf_stats *stats);
int glf_multi_image_processing_rgbf32_signals(glf_multi *w, const glf_options *opt, const float *h_rgb, int width, int height, int nsig,
                                              const float *h_sig, float *h_sig_out, float *h_out_rgb, double *eigvals_out,
                                              glf_stats *stats);

/* EntireComputation, hpc/image_processing.c:155-181 (-no_approx): z = clamp(y - L y) with the full N x N
 * Laplacian of ComputeEntireAffinityMatrix / ComputeEntireLaplacianMatrix / ComputeResultFromEntireLaplacian
 * (hpc/affinity.c:264-336, hpc/laplacian.c:44-65, hpc/display.c:128-149). The matrices are never stored
 * ((L y)_i = alpha (D_i y_i - (K y)_i)); O(N^2) work, limited to 4 Mpixel. d_zf, alpha_out optional. */
int glf_EntireComputation(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int kernel, float h_loc, float h_val,
                          uint8_t *d_out, float *d_zf, double *alpha_out);

/* ---- image I/O (host) -------------------------------------------------------------- */
/* int read_png(const char*, png_bytep** rows, int* w, int* h)  hpc/read_img.h:3, hpc/read_img.c:9-65
 * rows: malloc'd array of `height` malloc'd rows of `width` bytes (gray 8);
 * RGB / RGBA are converted to gray with libpng's default rgb_to_gray weights
 * (hpc/read_img.c:47-50). Returns 0 / -1. */
int glf_read_png(const char *filename, uint8_t ***row_pointers, int *width, int *height);
/* int write_png(const char*, png_bytep* rows, unsigned w, unsigned h)  hpc/write_img.h:4, hpc/write_img.c:5-53 */
int glf_write_png(const char *filename, uint8_t **img_bytes, unsigned width, unsigned height);
/* Colour (python/image_processing.py:410-432: the PoC filters the luma of an RGB image and keeps the chroma; the C reference
 * converts to gray on read): the same codec with rows of 3 * width bytes, R G B interleaved. */
int glf_read_png_rgb(const char *filename, uint8_t ***row_pointers, int *width, int *height);
int glf_write_png_rgb(const char *filename, uint8_t **img_bytes, unsigned width, unsigned height);
/* 16-bit greyscale (colour type 0, bit depth 16, non-interlaced): rows of `width` uint16_t values (host byte order; the file holds
 * them big-endian). glf_read_png16 rejects every other format (8-bit, RGB(A), palette, grey+alpha, interlaced) with -1, as
 * glf_read_png rejects 16-bit input. */
int glf_read_png16(const char *filename, uint16_t ***row_pointers, int *width, int *height);
int glf_write_png16(const char *filename, uint16_t **rows, unsigned width, unsigned height);
/* Greyscale Portable Float Map: the header "Pf\n<width> <height>\n<scale>\n" (any whitespace between the tokens, one whitespace
 * byte after the scale), then width * height raw floats, bottom row first; scale < 0: little-endian, > 0: big-endian. The reader takes
 * both byte orders and returns malloc'd rows top first; -1 for colour ("PF"), a short file, a zero or overflowing size or a malformed
 * header. The writer writes little-endian, scale -1.0. */
int glf_read_pfm(const char *filename, float ***rows, int *width, int *height);
int glf_write_pfm(const char *filename, float **rows, unsigned width, unsigned height);
/* Colour Portable Float Map: the header "PF", then 3 * width * height floats, rows of 3 * width interleaved R G B, bottom row first.
 * The reader takes both byte orders and returns malloc'd rows (3 * width floats each) top first; -1 for greyscale ("Pf"), a short file,
 * a zero or overflowing size or a malformed header. The writer writes little-endian, scale -1.0. */
int glf_read_pfm_rgb(const char *filename, float ***rows, int *width, int *height);
int glf_write_pfm_rgb(const char *filename, float **rows, unsigned width, unsigned height);

#ifdef __cplusplus
}
#endif
#endif /* GLF_H */
