/*
 * image_processing.c -- host shell of the MI355X-native graph-Laplacian filter.
 * Same entry point, flags, stage order, log lines and output files as the
 * reference's hpc/image_processing.c, with PETSc/SLEPc/MPI replaced by the HIP
 * C-ABI (include/glf.h) through the stage mirror in stages.h.
 *
 *   image_processing -f FILE [-num_eigvals N] [-opti_gs N] [-inv_it_epsilon E]
 *                    [-num_samples P | -sample_frac F] [-sampling uniform|random] [-sampling_seed S] [-fused] [-device D] [-no_approx] [-use_slepc]
 *                    [-dump_eigvecs] [-ngpu N [-ngpu_backend rccl|loopback]] [-filter_pow K]
 *                    [-kernel bilateral|photometric|spatial|nlm] [-h_loc X] [-h_val X] [-gain X] [-dump_residual]
 *                    [-filter reference|poc|smooth|sharpen [-sharpen_beta B]] [-color [-chroma | -rgb_graph]] [-depth16 | -float32 | -float_rgb] [-pix_band]
 *                    [-planes F1[,F2[,F3[,F4]]]]
 * -filter poc applies the Python PoC's active filter z = y - Phi diag(mu + 5) Phi^T y (python/image_processing.py:304-305) instead
 * of hpc/display.c:58-83; -filter smooth / sharpen the PoC's `smoothing` z = W y and `sharpening` z = (1 + B) W^2 y - B W^3 y
 * (python/image_processing.py:197-241, B = 1.5) with W = Phi diag(1 - mu) Phi^T from the eigenpairs this program computes.
 * -color keeps the colours of an RGB(A) input the way the PoC does (python/image_processing.py:410-432):
 * RGB -> YUV (python/utils.py:33-44), the luma plane is filtered, the chroma planes pass through, YUV -> RGB; the luma is
 * rounded to 8 bits first because every kernel here works on u8 pixel values (the PoC filters the unrounded floats).
 * -chroma (with -color) filters the two chroma planes too: the unrounded U and V go through the luma's graph with the same
 * -filter (glf_image_processing_signals), so chroma noise is smoothed along the luma's edges.
 * -rgb_graph (with -color) builds the graph from the RGB differences instead of the luma (glf_image_processing_rgb: the colour
 * bilateral kernel, which sees edges between colours of equal luma) and filters R, G and B through it with the same -filter.
 * -depth16 reads a 16-bit grey PNG and filters it on its 16-bit values (glf_image_processing_u16: the bilateral kernel with
 * v in 0..65535, -h_val in 16-bit units, 30 x 257 by default -- the 8-bit default graph on the same content) with the same
 * -filter, and writes results/input.png and results/output.png as 16-bit grey PNGs; -ngpu N works as for 8 bits.
 * -float32 reads a greyscale Portable Float Map ("Pf", either byte order) and filters it on its float values
 * (glf_image_processing_f32: the bilateral kernel on any finite value, -h_val in the image's own units, default 30) with the same
 * -filter, and writes results/input.pfm and results/output.pfm (the float z, not clamped); a NaN or an Inf in the file is refused.
 * It combines with -pix_band, -planes (the planes stay PNGs) and -ngpu N like -depth16, and with neither -depth16, -color, -no_approx
 * nor a -kernel other than bilateral.
 * -float_rgb reads a colour Portable Float Map ("PF", either byte order) and filters it on its three float channels
 * (glf_image_processing_rgbf32: the colour bilateral kernel on any finite values, -h_val in the image's own units, default 30) with the
 * same -filter, and writes results/input.pfm and results/output.pfm (both "PF"; the float z, not clamped); a NaN or an Inf in the file
 * is refused. It combines with -pix_band, -planes (grey PNGs) and -ngpu N like -float32, and with neither -color, -chroma, -rgb_graph, -depth16, -float32, -no_approx nor a -kernel option.
 * -pix_band (with -depth16, -float32 or -color -rgb_graph) sets the PIX_BAND tuning key: the 16-bit / colour kernel takes the band form
 * of the Nystroem stage and of the operator wherever the grey kernel would (GLF_PIX_BAND=1 in the environment does the same), and
 * one more line names the routes taken ("band form: nystroem_path 4, matvec_path 4", or the fallback's numbers).
 * -planes F1[,F2[,F3[,F4]]] (with -depth16, -float32 or -color -rgb_graph) is joint filtering: each file is a grey PNG of the image's size (16
 * or 8 bits; a depth map, an alpha matte, ...) whose pixel values go as a float plane through the 16-bit / colour image's graph with
 * the same -filter (glf_image_processing_u16_signals / glf_image_processing_rgb_signals; with -depth16 -ngpu N the glf_multi_ call).
 * Plane k (from 0) is written to results/plane_<k>.png at its input's bit depth as clamp(floor(z + 0.5)); results/output.png is the
 * one of the run without -planes. One more line says how many planes went through which graph.
 * -dump_residual writes results/residuals.png = |input - output| stretched to the full grey range, the PoC's residual image
 * (python/image_processing.py:378-380: plt.imsave of np.abs(y - z) with cmap 'gray' autoscales min..max).
 * -no_approx runs the full-matrix mode (hpc/image_processing.c:155-181); -use_slepc is accepted and refused.
 * -ngpu N is the reference's `mpirun -n N` (hpc/image_processing.c:30-38, 45-76): ONE process, N GPUs, one context and
 * one host thread per device, pixel rows sharded, RCCL collectives over xGMI issued by the library (glf_multi_*).
 * -ngpu_backend loopback runs the N ranks on one device with host-staged collectives (how the sharding is tested on a
 * one-GPU box). -filter_pow K: f(Pi) = Pi^K (the reference's MatPow(eigvals, 6) drops its result, hpc/utils.c:721, so the
 * default is K = 1; survey quirk Q3).
 *
 * The approximate path runs the tail the reference left commented out
 * (hpc/image_processing.c:240-275) as its specification (survey quirk Q1).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "stages.h"

static double wtime(void) /* MPI_Wtime */
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* ---- option database (PetscOptionsGet*, hpc/image_processing.c:82-154) ---------- */
static int g_argc;
static char **g_argv;

static const char *opt_value(const char *name)
{
    for (int i = 1; i + 1 < g_argc; ++i)
        if (strcmp(g_argv[i], name) == 0) return g_argv[i + 1];
    return NULL;
}
static int opt_has(const char *name)
{
    for (int i = 1; i < g_argc; ++i)
        if (strcmp(g_argv[i], name) == 0) return 1;
    return 0;
}

static void GetFilePath(char *filename, size_t len) /* :82-94 */
{
    const char *v = opt_value("-f");
    if (!v) {
        fprintf(stderr, "No filename found (option -f)\n");
        exit(1);
    }
    snprintf(filename, len, "%s", v);
}

static unsigned GetNumberEigenvalues(unsigned sample_size) /* :96-108 */
{
    const char *v = opt_value("-num_eigvals");
    long n = v ? strtol(v, NULL, 10) : -1;
    if (!v || n < 0 || n >= (long)sample_size) {
        n = (long)sample_size - 1;
        fprintf(stderr, "Invalid or invalid number of eigenvalues found (option -num_eigvals), so using %ld\n", n);
    }
    return (unsigned)n;
}

static int GetOptiGramSchmidt(void) /* :128-140 */
{
    const char *v = opt_value("-opti_gs");
    const long n = v ? strtol(v, NULL, 10) : 1;
    return n < 1 ? 1 : (int)n;
}

static double GetInverseIterationEpsilon(void) /* :142-154 */
{
    const char *v = opt_value("-inv_it_epsilon");
    return v ? strtod(v, NULL) : 0.1;
}

static unsigned GetRequestedSamples(unsigned width, unsigned height)
{
    const char *n = opt_value("-num_samples"), *f = opt_value("-sample_frac");
    if (n) return (unsigned)strtoul(n, NULL, 10);
    const double frac = f ? strtod(f, NULL) : 0.01; /* p = width*height*0.01, :187 */
    return (unsigned)(width * height * frac);
}

static void free_rows(png_bytep *rows, int height)
{
    if (!rows) return;
    for (int i = 0; i < height; ++i) free(rows[i]);
    free(rows);
}

/* ApproximationComputation, hpc/image_processing.c:183-277, stage by stage */
static png_bytep *ApproximationComputation(png_bytep *img_bytes, unsigned width, unsigned height)
{
    unsigned p = GetRequestedSamples(width, height);
    unsigned *sample_indices = NULL;
    Sampling((int)width, (int)height, &p, &sample_indices);
    if (!sample_indices || p < 2) {
        fprintf(stderr, "Sampling failed\n");
        return NULL;
    }
    printf("Sample size: %d\n", p);
    const unsigned m = GetNumberEigenvalues(p);

    double t = wtime();
    printf("Computing affinity matrices... ");
    Mat K_A = NULL, K_B = NULL;
    if (ComputeAffinityMatrices(&K_A, &K_B, img_bytes, (int)width, (int)height, p, sample_indices) != GLF_OK) goto fail;
    printf("%fs\n", wtime() - t);

    t = wtime();
    printf("Computing Laplacian matrices... ");
    Mat L_A = NULL, L_B = NULL;
    if (ComputeLaplacianMatrix(&L_A, &L_B, K_A, K_B) != GLF_OK) goto fail;
    printf("%fs\n", wtime() - t);
    MatDestroy(&K_A); /* K_B's tables are shared with L_B: destroyed at the end */

    t = wtime();
    Mat eigvals = NULL, eigvecs_A = NULL;
    printf("Computing %d smallest eigenvalues... ", m);
    if (opt_has("-use_slepc")) {
        fprintf(stderr, "-use_slepc: SLEPc is not part of this build; using the inverse subspace iteration\n");
    }
    const double epsilon = GetInverseIterationEpsilon();
    printf("(epsilon: %g) ", epsilon);
    if (InversePowerIteration(L_A, m, &eigvecs_A, &eigvals, GetOptiGramSchmidt(), epsilon) != GLF_OK) goto fail;
    printf("%fs\n", wtime() - t);
    printf("Inverse subspace iteration took %d outer iterations\n", LastEigStats()->outer_its);
    WriteDiagMat(eigvals, "results/eigenvalues_laplacian.txt");
    MatDestroy(&L_A);

    Mat eigvals_inv = InverseDiagMat(eigvals); /* :240 */
    t = wtime();
    printf("Computing Nystr\xc3\xb6m approximation... ");
    Mat eigvecs = Nystroem(L_B, eigvecs_A, eigvals_inv, width * height, p, m); /* :245 */
    if (!eigvecs) goto fail;
    printf("%fs\n", wtime() - t);
    MatDestroy(&eigvecs_A);
    MatDestroy(&eigvals_inv);
    MatDestroy(&L_B);

    Mat eigvecs_perm = Permutation(eigvecs, sample_indices, p); /* :251 */
    MatDestroy(&eigvecs);
    eigvecs = eigvecs_perm;
    if (!eigvecs) goto fail;

    if (opt_has("-dump_eigvecs")) { /* the diagnostics of hpc/image_processing.c:252-260 */
        char name[128];
        for (unsigned k = 0; k < 3 && k < m; ++k) {
            snprintf(name, sizeof(name), "results/eigenvector_%u_laplacian.txt", k);
            WriteMatCol(eigvecs, k, name);
            snprintf(name, sizeof(name), "results/eigenvector_%u_laplacian.png", k);
            WritePngMatCol(eigvecs, k, width, height, name);
        }
    }

    Mat f_eigvals = MatPow(eigvals, 6); /* :263, a no-op in the reference */
    MatDestroy(&eigvals);

    t = wtime();
    printf("Computing output image... ");
    png_bytep *output_img = ComputeResultFromLaplacian(img_bytes, eigvecs, f_eigvals, width, height); /* :269 */
    printf("%fs\n", wtime() - t);
    MatDestroy(&eigvecs);
    MatDestroy(&f_eigvals);
    MatDestroy(&K_B);
    free(sample_indices);
    return output_img;
fail:
    fprintf(stderr, "\nstage failed: %s\n", glf_ctx_last_error(glf_world()));
    free(sample_indices);
    return NULL;
}

/* EntireComputation, hpc/image_processing.c:155-181 (-no_approx): full N x N affinity and Laplacian,
 * z = clamp(y - L y). The matrices are never stored (glf_EntireComputation). */
static png_bytep *EntireComputation(png_bytep *img_bytes, unsigned width, unsigned height)
{
    glf_ctx *ctx = glf_world();
    const size_t n = (size_t)width * height;
    void *d_img = NULL, *d_out = NULL;
    uint8_t *flat = (uint8_t *)malloc(n);
    png_bytep *rows = NULL;
    if (!flat || glf_malloc(ctx, &d_img, n) != GLF_OK || glf_malloc(ctx, &d_out, n) != GLF_OK) goto out;
    for (unsigned r = 0; r < height; ++r) memcpy(flat + (size_t)r * width, img_bytes[r], width);
    if (glf_memcpy_h2d(ctx, d_img, flat, n) != GLF_OK) goto out;
    const double t = wtime();
    printf("Computing entire affinity matrix, Laplacian matrix and output image (matrices not stored)... ");
    const int rc = glf_EntireComputation(ctx, (const uint8_t *)d_img, (int)width, (int)height, stage_kernel, stage_h_loc, stage_h_val,
                                         (uint8_t *)d_out, NULL, NULL);
    if (rc != GLF_OK) {
        fprintf(stderr, "\nglf_EntireComputation: %s (%s)\n", glf_strerror(rc), glf_ctx_last_error(ctx));
        goto out;
    }
    printf("%fs\n", wtime() - t);
    if (glf_memcpy_d2h(ctx, flat, d_out, n) != GLF_OK) goto out;
    rows = (png_bytep *)malloc(sizeof(png_bytep) * height);
    for (unsigned r = 0; rows && r < height; ++r) {
        rows[r] = (png_bytep)malloc(width);
        memcpy(rows[r], flat + (size_t)r * width, width);
    }
out:
    free(flat);
    if (d_img) glf_free(ctx, d_img);
    if (d_out) glf_free(ctx, d_out);
    return rows;
}

static void fill_options(glf_options *opt, unsigned width, unsigned height)
{
    glf_options_default(opt);
    opt->num_samples = GetRequestedSamples(width, height);
    const char *v = opt_value("-num_eigvals");
    opt->num_eigvals = v ? (uint32_t)strtoul(v, NULL, 10) : 0;
    opt->opti_gs = GetOptiGramSchmidt();
    opt->epsilon = GetInverseIterationEpsilon();
    opt->kernel = stage_kernel;
    opt->sampling = stage_sampling;
    opt->sampling_seed = stage_sampling_seed;
    opt->h_loc = stage_h_loc;
    opt->h_val = stage_h_val;
    opt->gain = stage_gain;
    if ((v = opt_value("-filter_pow")) && atoi(v) > 0) opt->filter_pow = atoi(v);
    if ((v = opt_value("-filter"))) {
        if (strcmp(v, "poc") == 0) opt->filter_mode = GLF_FILTER_POC;
        else if (strcmp(v, "smooth") == 0) opt->filter_mode = GLF_FILTER_SMOOTH;
        else if (strcmp(v, "sharpen") == 0) opt->filter_mode = GLF_FILTER_SHARPEN;
    }
    if ((v = opt_value("-sharpen_beta"))) opt->filter_beta = (float)atof(v);
}

static void print_stage_times(const glf_stats *st, double epsilon)
{
    printf("Sample size: %d\n", st->p);
    printf("Computing affinity matrices... %fs\n", st->ms_affinity * 1e-3);
    printf("Computing Laplacian matrices... %fs\n", st->ms_laplacian * 1e-3);
    printf("Computing %d smallest eigenvalues... (epsilon: %g) %fs\n", st->m, epsilon, st->ms_eigen * 1e-3);
    printf("Inverse subspace iteration took %d outer iterations\n", st->eig.outer_its);
    printf("Computing Nystr\xc3\xb6m approximation... %fs\n", st->ms_nystroem * 1e-3);
    printf("Computing output image... %fs\n", st->ms_filter * 1e-3);
}

/* mpirun -n N (hpc/image_processing.c:30-76): N GPUs driven by this one process (glf_multi_*): the image is replicated on
 * every device, pixel rows are sharded, the result rows come back into one host image. */
static png_bytep *MultiComputation(png_bytep *img_bytes, unsigned width, unsigned height, int ngpu, int backend)
{
    glf_multi *world = NULL;
    int *devices = NULL;
    if (backend == GLF_MULTI_LOOPBACK) { /* every rank on the device of -device (default 0) */
        const char *dev = opt_value("-device");
        devices = (int *)malloc(sizeof(int) * (size_t)ngpu);
        for (int r = 0; devices && r < ngpu; ++r) devices[r] = dev ? atoi(dev) : 0;
    }
    int rc = glf_multi_create(&world, ngpu, devices, backend);
    free(devices);
    if (rc != GLF_OK) {
        fprintf(stderr, "glf_multi_create(%d GPUs, %s): %s\n", ngpu, backend == GLF_MULTI_RCCL ? "rccl" : "loopback", glf_strerror(rc));
        return NULL;
    }
    glf_options opt;
    fill_options(&opt, width, height);
    const size_t n = (size_t)width * height;
    uint8_t *flat = (uint8_t *)malloc(n), *flat_out = (uint8_t *)calloc(n, 1);
    glf_stats *st = (glf_stats *)calloc((size_t)ngpu, sizeof(glf_stats));
    png_bytep *rows = NULL;
    if (!flat || !flat_out || !st) goto out;
    for (unsigned r = 0; r < height; ++r) memcpy(flat + (size_t)r * width, img_bytes[r], width);
    rc = glf_multi_image_processing(world, &opt, flat, (int)width, (int)height, flat_out, NULL, NULL, st);
    if (rc != GLF_OK) {
        fprintf(stderr, "glf_multi_image_processing: %s (%s)\n", glf_strerror(rc), glf_multi_last_error(world));
        goto out;
    }
    print_stage_times(&st[0], opt.epsilon);
    for (int r = 0; r < ngpu; ++r) printf("rank %d: pixel rows [%d, %d), %.3f ms on the device\n", r, st[r].row0, st[r].row1, st[r].ms_total);
    rows = (png_bytep *)malloc(sizeof(png_bytep) * height);
    for (unsigned r = 0; rows && r < height; ++r) {
        rows[r] = (png_bytep)malloc(width);
        memcpy(rows[r], flat_out + (size_t)r * width, width);
    }
out:
    free(flat);
    free(flat_out);
    free(st);
    glf_multi_destroy(world);
    return rows;
}

/* -pix_band (with -depth16 or -color -rgb_graph): the band form of the 16-bit and colour kernels (the PIX_BAND tuning key) on a
 * context, and the line that names the routes the call took */
static void pix_band_set(glf_ctx *ctx)
{
    if (opt_has("-pix_band") && glf_ctx_set_tuning(ctx, "PIX_BAND", "1") != GLF_OK) fprintf(stderr, "-pix_band: could not set PIX_BAND\n");
}
static void pix_band_report(const glf_stats *st)
{
    if (opt_has("-pix_band")) printf("band form: nystroem_path %d, matvec_path %d\n", (int)st->nystroem_path, (int)st->matvec_path);
}

/* -planes: up to GLF_MAX_SIGNALS grey PNGs of the image's size as float planes [nsig][height*width]. A file that cannot be read or
 * has another size ends the program with status 1. */
static int g_nplanes;
static int g_plane_bits[GLF_MAX_SIGNALS];
static float *g_planes, *g_planes_out;

static void planes_fail(void)
{
    FinalizeProgram();
    exit(1);
}

static void planes_load(unsigned width, unsigned height)
{
    const char *v = opt_value("-planes");
    if (!v) return;
    const size_t n = (size_t)width * height;
    char *list = strdup(v);
    g_planes = (float *)malloc(sizeof(float) * GLF_MAX_SIGNALS * n);
    g_planes_out = (float *)calloc(GLF_MAX_SIGNALS * n, sizeof(float));
    if (!list || !g_planes || !g_planes_out) {
        fprintf(stderr, "-planes: out of memory\n");
        planes_fail();
    }
    for (char *name = strtok(list, ","); name; name = strtok(NULL, ",")) {
        if (g_nplanes == GLF_MAX_SIGNALS) {
            fprintf(stderr, "-planes takes at most %d files\n", GLF_MAX_SIGNALS);
            planes_fail();
        }
        float *dst = g_planes + (size_t)g_nplanes * n;
        uint16_t **r16 = NULL;
        uint8_t **r8 = NULL;
        int w = 0, h = 0;
        if (glf_read_png16(name, &r16, &w, &h) == 0) g_plane_bits[g_nplanes] = 16;
        else if (glf_read_png(name, &r8, &w, &h) == 0) g_plane_bits[g_nplanes] = 8;
        else {
            fprintf(stderr, "-planes: could not read %s as a grey PNG\n", name);
            planes_fail();
        }
        if (w != (int)width || h != (int)height) {
            fprintf(stderr, "-planes: %s is %dx%d, the image %ux%u\n", name, w, h, width, height);
            planes_fail();
        }
        for (unsigned r = 0; r < height; ++r)
            for (unsigned c = 0; c < width; ++c) dst[(size_t)r * width + c] = r16 ? (float)r16[r][c] : (float)r8[r][c];
        for (int r = 0; r < h; ++r) free(r16 ? (void *)r16[r] : (void *)r8[r]);
        free(r16 ? (void *)r16 : (void *)r8);
        ++g_nplanes;
    }
    free(list);
    if (g_nplanes == 0) {
        fprintf(stderr, "-planes needs at least one file\n");
        planes_fail();
    }
}

/* results/plane_<k>.png = clamp(floor(z_k + 0.5)) at the input plane's bit depth; returns 0, or 4 when a file could not be written */
static int planes_write(unsigned width, unsigned height, const char *graph)
{
    const size_t n = (size_t)width * height;
    int status = 0;
    for (int k = 0; k < g_nplanes; ++k) {
        const float *z = g_planes_out + (size_t)k * n;
        const double vmax = g_plane_bits[k] == 16 ? 65535.0 : 255.0;
        char name[64];
        snprintf(name, sizeof(name), "results/plane_%d.png", k);
        void **rows = (void **)calloc(height, sizeof(void *));
        for (unsigned r = 0; rows && r < height; ++r) {
            rows[r] = malloc((size_t)width * (g_plane_bits[k] == 16 ? 2 : 1));
            for (unsigned c = 0; rows[r] && c < width; ++c) {
                double x = floor((double)z[(size_t)r * width + c] + 0.5);
                x = x >= 0.0 ? (x > vmax ? vmax : x) : 0.0;
                if (g_plane_bits[k] == 16) ((uint16_t *)rows[r])[c] = (uint16_t)x;
                else ((uint8_t *)rows[r])[c] = (uint8_t)x;
            }
        }
        if (!rows || (g_plane_bits[k] == 16 ? glf_write_png16(name, (uint16_t **)rows, width, height)
                                            : glf_write_png(name, (uint8_t **)rows, width, height)) != 0)
            status = 4;
        for (unsigned r = 0; rows && r < height; ++r) free(rows[r]);
        free(rows);
    }
    printf("Planes: %d plane%s filtered through the %s graph (filter %s)\n", g_nplanes, g_nplanes == 1 ? "" : "s", graph,
           opt_value("-filter") ? opt_value("-filter") : "reference");
    return status;
}

/* -depth16 / -float32 / -float_rgb: img (rows of `width` uint16_t; float with f32 = 1; 3 interleaved floats with f32 = 2) through
 * glf_image_processing_u16 / _f32 / _rgbf32 on one context, or the glf_multi_ call on ngpu ranks; returns the output rows in the
 * input's format (NULL on failure, the message printed). */
static void **DeepComputation(void **img, unsigned width, unsigned height, int ngpu, int backend, int f32)
{
    const size_t n = (size_t)width * height, esz = f32 == 2 ? 3 * sizeof(float) : f32 ? sizeof(float) : sizeof(uint16_t); /* bytes per pixel */
    const char *fn = f32 == 2 ? "glf_image_processing_rgbf32" : f32 ? "glf_image_processing_f32" : "glf_image_processing_u16";
    void *flat = malloc(esz * n), *flat_out = calloc(n, esz);
    void **rows = NULL;
    glf_options opt;
    fill_options(&opt, width, height);
    int ok = flat && flat_out;
    for (unsigned r = 0; ok && r < height; ++r) memcpy((char *)flat + esz * r * width, img[r], esz * width);
    if (ok && ngpu > 0) {
        glf_multi *world = NULL;
        int *devices = NULL;
        if (backend == GLF_MULTI_LOOPBACK) { /* every rank on the device of -device (default 0) */
            const char *dev = opt_value("-device");
            devices = (int *)malloc(sizeof(int) * (size_t)ngpu);
            for (int r = 0; devices && r < ngpu; ++r) devices[r] = dev ? atoi(dev) : 0;
        }
        int rc = glf_multi_create(&world, ngpu, devices, backend);
        free(devices);
        glf_stats *st = (glf_stats *)calloc((size_t)ngpu, sizeof(glf_stats));
        if (rc != GLF_OK) fprintf(stderr, "glf_multi_create(%d GPUs, %s): %s\n", ngpu, backend == GLF_MULTI_RCCL ? "rccl" : "loopback", glf_strerror(rc));
        else if (st) {
            for (int r = 0; r < ngpu; ++r) pix_band_set(glf_multi_ctx(world, r));
            if (f32 == 2)
                rc = g_nplanes ? glf_multi_image_processing_rgbf32_signals(world, &opt, (const float *)flat, (int)width, (int)height, g_nplanes,
                                                                           g_planes, g_planes_out, (float *)flat_out, NULL, st)
                               : glf_multi_image_processing_rgbf32(world, &opt, (const float *)flat, (int)width, (int)height, (float *)flat_out, NULL, st);
            else if (f32)
                rc = g_nplanes ? glf_multi_image_processing_f32_signals(world, &opt, (const float *)flat, (int)width, (int)height, g_nplanes, g_planes,
                                                                        g_planes_out, (float *)flat_out, NULL, st)
                               : glf_multi_image_processing_f32(world, &opt, (const float *)flat, (int)width, (int)height, (float *)flat_out, NULL, st);
            else
                rc = g_nplanes ? glf_multi_image_processing_u16_signals(world, &opt, (const uint16_t *)flat, (int)width, (int)height, g_nplanes, g_planes,
                                                                        g_planes_out, (uint16_t *)flat_out, NULL, NULL, st)
                               : glf_multi_image_processing_u16(world, &opt, (const uint16_t *)flat, (int)width, (int)height, (uint16_t *)flat_out, NULL,
                                                                NULL, st);
            if (rc != GLF_OK)
                fprintf(stderr, "%s: %s (%s)\n", f32 == 2 ? "glf_multi_image_processing_rgbf32" : f32 ? "glf_multi_image_processing_f32" : "glf_multi_image_processing_u16",
                        glf_strerror(rc), glf_multi_last_error(world));
            else {
                print_stage_times(&st[0], opt.epsilon);
                pix_band_report(&st[0]);
                for (int r = 0; r < ngpu; ++r)
                    printf("rank %d: pixel rows [%d, %d), %.3f ms on the device\n", r, st[r].row0, st[r].row1, st[r].ms_total);
            }
        }
        ok = rc == GLF_OK && st;
        free(st);
        if (world) glf_multi_destroy(world);
    } else if (ok) {
        glf_ctx *ctx = glf_world();
        void *d_img = NULL, *d_out = NULL, *d_sig = NULL, *d_sig_out = NULL;
        const size_t sig_bytes = sizeof(float) * n * (size_t)g_nplanes;
        glf_stats st;
        ok = glf_malloc(ctx, &d_img, esz * n) == GLF_OK && glf_malloc(ctx, &d_out, esz * n) == GLF_OK &&
             glf_memcpy_h2d(ctx, d_img, flat, esz * n) == GLF_OK;
        if (ok && g_nplanes)
            ok = glf_malloc(ctx, &d_sig, sig_bytes) == GLF_OK && glf_malloc(ctx, &d_sig_out, sig_bytes) == GLF_OK &&
                 glf_memcpy_h2d(ctx, d_sig, g_planes, sig_bytes) == GLF_OK;
        if (ok) {
            pix_band_set(ctx);
            int rc;
            if (f32 == 2)
                rc = g_nplanes ? glf_image_processing_rgbf32_signals(ctx, &opt, (const float *)d_img, (int)width, (int)height, g_nplanes,
                                                                     (const float *)d_sig, (float *)d_sig_out, (float *)d_out, NULL, &st)
                               : glf_image_processing_rgbf32(ctx, &opt, (const float *)d_img, (int)width, (int)height, (float *)d_out, NULL, &st);
            else if (f32)
                rc = g_nplanes ? glf_image_processing_f32_signals(ctx, &opt, (const float *)d_img, (int)width, (int)height, g_nplanes, (const float *)d_sig,
                                                                  (float *)d_sig_out, (float *)d_out, NULL, &st)
                               : glf_image_processing_f32(ctx, &opt, (const float *)d_img, (int)width, (int)height, (float *)d_out, NULL, &st);
            else
                rc = g_nplanes ? glf_image_processing_u16_signals(ctx, &opt, (const uint16_t *)d_img, (int)width, (int)height, g_nplanes,
                                                                  (const float *)d_sig, (float *)d_sig_out, (uint16_t *)d_out, NULL, NULL, &st)
                               : glf_image_processing_u16(ctx, &opt, (const uint16_t *)d_img, (int)width, (int)height, (uint16_t *)d_out, NULL, NULL, &st);
            if (rc != GLF_OK) fprintf(stderr, "%s: %s (%s)\n", fn, glf_strerror(rc), glf_ctx_last_error(ctx));
            ok = rc == GLF_OK && glf_memcpy_d2h(ctx, flat_out, d_out, esz * n) == GLF_OK &&
                 (!g_nplanes || glf_memcpy_d2h(ctx, g_planes_out, d_sig_out, sig_bytes) == GLF_OK);
            if (ok) {
                print_stage_times(&st, opt.epsilon);
                pix_band_report(&st);
            }
        }
        if (d_img) glf_free(ctx, d_img);
        if (d_out) glf_free(ctx, d_out);
        if (d_sig) glf_free(ctx, d_sig);
        if (d_sig_out) glf_free(ctx, d_sig_out);
    }
    if (ok) {
        rows = (void **)calloc(height, sizeof(void *));
        for (unsigned r = 0; rows && r < height; ++r) {
            rows[r] = malloc(esz * width);
            if (rows[r]) memcpy(rows[r], (char *)flat_out + esz * r * width, esz * width);
        }
    }
    free(flat);
    free(flat_out);
    return rows;
}

static void free_rows16(void *rows_, int height) /* (rows of any element type) */
{
    void **rows = (void **)rows_;
    if (!rows) return;
    for (int r = 0; r < height; ++r) free(rows[r]);
    free(rows);
}

/* -color (python/image_processing.py:410-432): filter the luma of an RGB image, keep its chroma. Returns rows of 3 * width
 * bytes for glf_write_png_rgb; *input_rgb receives the input as read (for results/input.png). */
static const double yuv_from_rgb[3][3] = {{0.299, 0.587, 0.114},                 /* python/utils.py:33-36 (the BT.601 YUV matrix) */
                                          {-0.14714119, -0.28886916, 0.43601035},
                                          {0.61497538, -0.51496512, -0.10001026}};
static png_bytep *ColorComputation(const char *filename, unsigned *width_out, unsigned *height_out, png_bytep **input_rgb)
{
    int w = 0, h = 0;
    png_bytep *rgb = NULL, *rows = NULL;
    if (glf_read_png_rgb(filename, &rgb, &w, &h) != 0) return NULL;
    *width_out = (unsigned)w;
    *height_out = (unsigned)h;
    *input_rgb = rgb;
    const size_t n = (size_t)w * h;
    if (opt_has("-rgb_graph")) { /* the colour graph: R, G, B through the operator built from the RGB differences */
        printf("Read image %s of size %dx%d => %d pixels (colour: graph from the RGB differences, R, G, B filtered)\n", filename, w, h, w * h);
        glf_ctx *cctx = glf_world();
        uint8_t *flat = (uint8_t *)malloc(3 * n);
        void *d_rgb = NULL, *d_rgb_out = NULL, *d_sig = NULL, *d_sig_out = NULL;
        glf_options copt;
        glf_stats cst;
        fill_options(&copt, (unsigned)w, (unsigned)h);
        planes_load((unsigned)w, (unsigned)h);
        const size_t sig_bytes = sizeof(float) * n * (size_t)g_nplanes;
        int ok = flat && glf_malloc(cctx, &d_rgb, 3 * n) == GLF_OK && glf_malloc(cctx, &d_rgb_out, 3 * n) == GLF_OK;
        for (int r = 0; ok && r < h; ++r) memcpy(flat + (size_t)r * 3 * w, rgb[r], 3 * (size_t)w);
        ok = ok && glf_memcpy_h2d(cctx, d_rgb, flat, 3 * n) == GLF_OK;
        if (ok && g_nplanes)
            ok = glf_malloc(cctx, &d_sig, sig_bytes) == GLF_OK && glf_malloc(cctx, &d_sig_out, sig_bytes) == GLF_OK &&
                 glf_memcpy_h2d(cctx, d_sig, g_planes, sig_bytes) == GLF_OK;
        if (ok) {
            pix_band_set(cctx);
            const int rc = g_nplanes ? glf_image_processing_rgb_signals(cctx, &copt, (const uint8_t *)d_rgb, w, h, g_nplanes, (const float *)d_sig,
                                                                        (float *)d_sig_out, (uint8_t *)d_rgb_out, NULL, NULL, &cst)
                                     : glf_image_processing_rgb(cctx, &copt, (const uint8_t *)d_rgb, w, h, (uint8_t *)d_rgb_out, NULL, NULL, &cst);
            if (rc != GLF_OK) fprintf(stderr, "glf_image_processing_rgb: %s (%s)\n", glf_strerror(rc), glf_ctx_last_error(cctx));
            ok = rc == GLF_OK && glf_memcpy_d2h(cctx, flat, d_rgb_out, 3 * n) == GLF_OK &&
                 (!g_nplanes || glf_memcpy_d2h(cctx, g_planes_out, d_sig_out, sig_bytes) == GLF_OK);
        }
        if (d_sig) glf_free(cctx, d_sig);
        if (d_sig_out) glf_free(cctx, d_sig_out);
        if (ok) {
            print_stage_times(&cst, copt.epsilon);
            pix_band_report(&cst);
            rows = (png_bytep *)malloc(sizeof(png_bytep) * (size_t)h);
            for (int r = 0; rows && r < h; ++r) {
                rows[r] = (png_bytep)malloc(3 * (size_t)w);
                if (rows[r]) memcpy(rows[r], flat + (size_t)r * 3 * w, 3 * (size_t)w);
            }
        }
        free(flat);
        if (d_rgb) glf_free(cctx, d_rgb);
        if (d_rgb_out) glf_free(cctx, d_rgb_out);
        return rows;
    }
    printf("Read image %s of size %dx%d => %d pixels (colour: the luma plane is filtered)\n", filename, w, h, w * h);
    /* rgb_from_yuv = inv(yuv_from_rgb), python/utils.py:38 */
    double inv[3][3];
    {
        const double(*a)[3] = yuv_from_rgb;
        const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
                inv[i][j] = (a[r0][c0] * a[r1][c1] - a[r0][c1] * a[r1][c0]) / det;
            }
    }
    const int chroma = opt_has("-chroma");
    double *yuv = (double *)malloc(sizeof(double) * 3 * n);
    uint8_t *luma = (uint8_t *)malloc(n);
    float *zf = (float *)malloc(sizeof(float) * n);
    float *uv = chroma ? (float *)malloc(sizeof(float) * 2 * n) : NULL; /* U, V as float; filtered in place */
    glf_ctx *ctx = glf_world();
    void *d_img = NULL, *d_out = NULL, *d_zf = NULL, *d_uv = NULL, *d_uv_out = NULL;
    if (!yuv || !luma || !zf || (chroma && !uv)) goto out;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const double R = rgb[r][3 * c], G = rgb[r][3 * c + 1], B = rgb[r][3 * c + 2];
            const size_t i = (size_t)r * w + c;
            for (int k = 0; k < 3; ++k) yuv[k * n + i] = R * yuv_from_rgb[k][0] + G * yuv_from_rgb[k][1] + B * yuv_from_rgb[k][2]; /* rgb2ycc */
            double y = yuv[i] + 0.5;
            luma[i] = (uint8_t)(y < 0.0 ? 0.0 : (y > 255.0 ? 255.0 : y));
        }
    if (glf_malloc(ctx, &d_img, n) != GLF_OK || glf_malloc(ctx, &d_out, n) != GLF_OK || glf_malloc(ctx, &d_zf, sizeof(float) * n) != GLF_OK) goto out;
    if (glf_memcpy_h2d(ctx, d_img, luma, n) != GLF_OK) goto out;
    if (chroma) {
        for (size_t i = 0; i < 2 * n; ++i) uv[i] = (float)yuv[n + i];
        if (glf_malloc(ctx, &d_uv, sizeof(float) * 2 * n) != GLF_OK || glf_malloc(ctx, &d_uv_out, sizeof(float) * 2 * n) != GLF_OK) goto out;
        if (glf_memcpy_h2d(ctx, d_uv, uv, sizeof(float) * 2 * n) != GLF_OK) goto out;
    }
    glf_options opt;
    fill_options(&opt, (unsigned)w, (unsigned)h);
    glf_stats st;
    {
        const int rc = chroma ? glf_image_processing_signals(ctx, &opt, (const uint8_t *)d_img, w, h, 2, (const float *)d_uv, (float *)d_uv_out,
                                                             (uint8_t *)d_out, (float *)d_zf, NULL, &st)
                              : glf_image_processing(ctx, &opt, (const uint8_t *)d_img, w, h, (uint8_t *)d_out, (float *)d_zf, NULL, &st);
        if (rc != GLF_OK) {
            fprintf(stderr, "%s: %s (%s)\n", chroma ? "glf_image_processing_signals" : "glf_image_processing", glf_strerror(rc),
                    glf_ctx_last_error(ctx));
            goto out;
        }
    }
    print_stage_times(&st, opt.epsilon);
    if (glf_memcpy_d2h(ctx, zf, d_zf, sizeof(float) * n) != GLF_OK) goto out;
    if (chroma) {
        if (glf_memcpy_d2h(ctx, uv, d_uv_out, sizeof(float) * 2 * n) != GLF_OK) goto out;
        printf("Chroma: the U and V planes were filtered through the luma's graph (filter %s)\n",
               opt_value("-filter") ? opt_value("-filter") : "reference");
    }
    rows = (png_bytep *)malloc(sizeof(png_bytep) * (size_t)h);
    for (int r = 0; rows && r < h; ++r) {
        rows[r] = (png_bytep)malloc(3 * (size_t)w);
        for (int c = 0; rows[r] && c < w; ++c) {
            const size_t i = (size_t)r * w + c;
            const double zy = (double)zf[i];                                       /* z[:, :, 0] = z_ycc; chroma unchanged */
            const double u = chroma ? (double)uv[i] : yuv[n + i], v = chroma ? (double)uv[n + i] : yuv[2 * n + i]; /* (or filtered) */
            for (int k = 0; k < 3; ++k) {                                          /* ycc2rgb, then astype(uint8) made safe */
                double x = zy * inv[k][0] + u * inv[k][1] + v * inv[k][2];
                x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
                rows[r][3 * c + k] = (png_byte)x;
            }
        }
    }
out:
    free(yuv);
    free(luma);
    free(zf);
    free(uv);
    if (d_uv) glf_free(ctx, d_uv);
    if (d_uv_out) glf_free(ctx, d_uv_out);
    if (d_img) glf_free(ctx, d_img);
    if (d_out) glf_free(ctx, d_out);
    if (d_zf) glf_free(ctx, d_zf);
    return rows;
}

/* Same path through the single fused entry point (no stage materialisation:
 * Phi is written in raster order directly and K_A is never stored). */
static png_bytep *FusedComputation(png_bytep *img_bytes, unsigned width, unsigned height)
{
    glf_ctx *ctx = glf_world();
    glf_options opt;
    fill_options(&opt, width, height);
    const size_t n = (size_t)width * height;
    void *d_img = NULL, *d_out = NULL;
    uint8_t *flat = (uint8_t *)malloc(n);
    png_bytep *rows = NULL;
    if (!flat || glf_malloc(ctx, &d_img, n) != GLF_OK || glf_malloc(ctx, &d_out, n) != GLF_OK) goto out;
    for (unsigned r = 0; r < height; ++r) memcpy(flat + (size_t)r * width, img_bytes[r], width);
    if (glf_memcpy_h2d(ctx, d_img, flat, n) != GLF_OK) goto out;
    glf_stats st;
    const int rc = glf_image_processing(ctx, &opt, (const uint8_t *)d_img, (int)width, (int)height, (uint8_t *)d_out, NULL, NULL, &st);
    if (rc != GLF_OK) {
        fprintf(stderr, "glf_image_processing: %s (%s)\n", glf_strerror(rc), glf_ctx_last_error(ctx));
        goto out;
    }
    print_stage_times(&st, opt.epsilon);
    if (glf_memcpy_d2h(ctx, flat, d_out, n) != GLF_OK) goto out;
    rows = (png_bytep *)malloc(sizeof(png_bytep) * height);
    for (unsigned r = 0; rows && r < height; ++r) {
        rows[r] = (png_bytep)malloc(width);
        memcpy(rows[r], flat + (size_t)r * width, width);
    }
out:
    free(flat);
    if (d_img) glf_free(ctx, d_img);
    if (d_out) glf_free(ctx, d_out);
    return rows;
}

int main(int argc, char **argv)
{
    g_argc = argc;
    g_argv = argv;
    char filename[4096];
    const char *dev = opt_value("-device");
    if (InitProgram(dev ? atoi(dev) : 0) != GLF_OK) return 2; /* :284 */
    const double start_time = wtime();
    const char *ng = opt_value("-ngpu"), *nb = opt_value("-ngpu_backend");
    const int ngpu = ng ? atoi(ng) : 0; /* 0: the single-context paths below */
    if (ng && ngpu < 1) {
        fprintf(stderr, "-ngpu needs a positive device count\n");
        FinalizeProgram();
        return 1;
    }
    printf("Running with %d processes\n", ngpu > 0 ? ngpu : 1); /* :286: here a "process" is a GPU rank of this one process */
    { /* additions: the reference's constants as flags, same defaults */
        const char *v;
        if ((v = opt_value("-h_loc")) && atof(v) > 0.0) stage_h_loc = (float)atof(v);
        if ((v = opt_value("-h_val")) && atof(v) > 0.0) stage_h_val = (float)atof(v);
        if ((v = opt_value("-gain"))) stage_gain = (float)atof(v);
        if ((v = opt_value("-sampling"))) { /* the PoC's sampler registry, python/sampling/__init__.py:4-9 (the C reference has the grid only) */
            if (strcmp(v, "uniform") == 0 || strcmp(v, "spatially_uniform") == 0) stage_sampling = GLF_SAMPLING_UNIFORM;
            else if (strcmp(v, "random") == 0) stage_sampling = GLF_SAMPLING_RANDOM;
            else {
                fprintf(stderr, "-sampling %s: expected uniform or random\n", v);
                FinalizeProgram();
                return 1;
            }
        }
        if ((v = opt_value("-sampling_seed"))) stage_sampling_seed = strtoull(v, NULL, 10);
        if ((v = opt_value("-kernel"))) { /* bilateral (hpc/affinity.c:121) | photometric | spatial (:119-120) | nlm (python/affinity_methods/NLM.py) */
            if (strcmp(v, "bilateral") == 0) stage_kernel = GLF_KERNEL_BILATERAL;
            else if (strcmp(v, "photometric") == 0) stage_kernel = GLF_KERNEL_PHOTOMETRIC;
            else if (strcmp(v, "spatial") == 0) stage_kernel = GLF_KERNEL_SPATIAL;
            else if (strcmp(v, "nlm") == 0) {
                stage_kernel = GLF_KERNEL_NLM;
                if (!opt_value("-h_val")) stage_h_val = 3.0f; /* the PoC's h (NLM.py:12) */
            } else {
                fprintf(stderr, "-kernel %s: expected bilateral, photometric, spatial or nlm\n", v);
                FinalizeProgram();
                return 1;
            }
        }
    }
    GetFilePath(filename, sizeof(filename));

    int width = 0, height = 0;
    png_bytep *img_bytes = NULL, *output_img = NULL;
    if (opt_has("-depth16")) {
        const char *other = opt_has("-color") ? "-color" : opt_has("-chroma") ? "-chroma" : opt_has("-rgb_graph") ? "-rgb_graph"
                          : opt_has("-no_approx") ? "-no_approx" : NULL;
        if (other) {
            fprintf(stderr, "-depth16 filters a 16-bit grey image: it cannot be combined with %s\n", other);
            FinalizeProgram();
            return 1;
        }
    }
    if (opt_has("-float32")) {
        const char *kv = opt_value("-kernel");
        const char *other = opt_has("-color") ? "-color" : opt_has("-chroma") ? "-chroma" : opt_has("-rgb_graph") ? "-rgb_graph"
                          : opt_has("-no_approx") ? "-no_approx" : opt_has("-depth16") ? "-depth16"
                          : (kv && strcmp(kv, "bilateral") != 0) ? "-kernel" : NULL;
        if (other) {
            fprintf(stderr, strcmp(other, "-kernel") == 0 ? "-float32 filters a float grey image with the bilateral kernel: it cannot be combined with %s %s\n"
                                                          : "-float32 filters a float grey image: it cannot be combined with %s%s\n",
                    other, strcmp(other, "-kernel") == 0 ? kv : "");
            FinalizeProgram();
            return 1;
        }
    }
    if (opt_has("-float_rgb")) {
        const char *kv = opt_value("-kernel");
        const char *other = opt_has("-color") ? "-color" : opt_has("-chroma") ? "-chroma" : opt_has("-rgb_graph") ? "-rgb_graph"
                          : opt_has("-depth16") ? "-depth16" : opt_has("-float32") ? "-float32" : opt_has("-no_approx") ? "-no_approx"
                          : opt_has("-kernel") ? "-kernel" : NULL;
        if (other) {
            fprintf(stderr, strcmp(other, "-kernel") == 0 ? "-float_rgb filters a float colour image with its own bilateral kernel: it cannot be combined with %s %s\n"
                                                          : "-float_rgb filters a float colour image: it cannot be combined with %s%s\n",
                    other, strcmp(other, "-kernel") == 0 ? (kv ? kv : "") : "");
            FinalizeProgram();
            return 1;
        }
    }
    if (opt_has("-chroma") && !opt_has("-color")) {
        fprintf(stderr, "-chroma filters the chroma planes of a colour image: it needs -color\n");
        FinalizeProgram();
        return 1;
    }
    if (opt_has("-rgb_graph") && (!opt_has("-color") || opt_has("-chroma"))) {
        fprintf(stderr, opt_has("-color") ? "-rgb_graph filters R, G and B through the colour graph: it cannot be combined with -chroma\n"
                                          : "-rgb_graph builds the graph of a colour image: it needs -color\n");
        FinalizeProgram();
        return 1;
    }
    if (opt_has("-pix_band") && !opt_has("-depth16") && !opt_has("-float32") && !opt_has("-float_rgb") && !opt_has("-rgb_graph")) {
        fprintf(stderr, "-pix_band selects the band form of the 16-bit, float and colour kernels: it needs -depth16 or -color -rgb_graph (or -float32), or -float_rgb\n");
        FinalizeProgram();
        return 1;
    }
    if (opt_has("-planes") && !opt_has("-depth16") && !opt_has("-float32") && !opt_has("-float_rgb") && !(opt_has("-color") && opt_has("-rgb_graph"))) {
        fprintf(stderr, "-planes filters extra planes through the 16-bit, the float or the colour graph: it needs -depth16 or -color -rgb_graph (or -float32), or -float_rgb\n");
        FinalizeProgram();
        return 1;
    }
    if (opt_has("-depth16")) { /* 16-bit grey: its own reader, route and writer */
        uint16_t **in16 = NULL, **out16 = NULL;
        if (glf_read_png16(filename, &in16, &width, &height) != 0) {
            uint8_t **in8 = NULL;
            int w8 = 0, h8 = 0;
            if (read_png(filename, &in8, &w8, &h8) == 0) {
                fprintf(stderr, "-depth16 needs a 16-bit grey PNG: %s is an 8-bit image\n", filename);
                free_rows(in8, h8);
            } else
                fprintf(stderr, "Could not read %s as a 16-bit gray PNG\n", filename);
            FinalizeProgram();
            return 1;
        }
        if (!opt_value("-h_val")) stage_h_val = 30.0f * 257.0f; /* the 8-bit default graph on the same content */
        printf("Read image %s of size %dx%d => %d pixels (16-bit gray)\n", filename, width, height, width * height);
        planes_load((unsigned)width, (unsigned)height);
        out16 = (uint16_t **)DeepComputation((void **)in16, (unsigned)width, (unsigned)height, ngpu,
                                             nb && strcmp(nb, "loopback") == 0 ? GLF_MULTI_LOOPBACK : GLF_MULTI_RCCL, 0);
        int dstatus = out16 ? 0 : 5;
        if (glf_write_png16("results/input.png", in16, (unsigned)width, (unsigned)height) != 0) dstatus = dstatus ? dstatus : 4;
        if (out16 && glf_write_png16("results/output.png", out16, (unsigned)width, (unsigned)height) != 0) dstatus = dstatus ? dstatus : 4;
        if (out16 && g_nplanes && planes_write((unsigned)width, (unsigned)height, "16-bit") != 0) dstatus = dstatus ? dstatus : 4;
        printf("Total computation time: %fs\n", wtime() - start_time);
        free_rows16(in16, height);
        free_rows16(out16, height);
        FinalizeProgram();
        return dstatus;
    }
    if (opt_has("-float32")) { /* float grey: a PFM in, a PFM out */
        float **in32 = NULL, **out32 = NULL;
        if (glf_read_pfm(filename, &in32, &width, &height) != 0) {
            fprintf(stderr, "-float32 needs a greyscale Portable Float Map (Pf): could not read %s as one\n", filename);
            FinalizeProgram();
            return 1;
        }
        printf("Read image %s of size %dx%d => %d pixels (32-bit float gray)\n", filename, width, height, width * height);
        planes_load((unsigned)width, (unsigned)height);
        out32 = (float **)DeepComputation((void **)in32, (unsigned)width, (unsigned)height, ngpu,
                                          nb && strcmp(nb, "loopback") == 0 ? GLF_MULTI_LOOPBACK : GLF_MULTI_RCCL, 1);
        int fstatus = out32 ? 0 : 5;
        if (glf_write_pfm("results/input.pfm", in32, (unsigned)width, (unsigned)height) != 0) fstatus = fstatus ? fstatus : 4;
        if (out32 && glf_write_pfm("results/output.pfm", out32, (unsigned)width, (unsigned)height) != 0) fstatus = fstatus ? fstatus : 4;
        if (out32 && g_nplanes && planes_write((unsigned)width, (unsigned)height, "float") != 0) fstatus = fstatus ? fstatus : 4;
        printf("Total computation time: %fs\n", wtime() - start_time);
        free_rows16(in32, height);
        free_rows16(out32, height);
        FinalizeProgram();
        return fstatus;
    }
    if (opt_has("-float_rgb")) { /* float colour: a "PF" PFM in, a "PF" PFM out */
        float **in96 = NULL, **out96 = NULL;
        if (glf_read_pfm_rgb(filename, &in96, &width, &height) != 0) {
            fprintf(stderr, "-float_rgb needs a colour Portable Float Map (PF): could not read %s as one\n", filename);
            FinalizeProgram();
            return 1;
        }
        printf("Read image %s of size %dx%d => %d pixels (32-bit float colour)\n", filename, width, height, width * height);
        planes_load((unsigned)width, (unsigned)height);
        out96 = (float **)DeepComputation((void **)in96, (unsigned)width, (unsigned)height, ngpu,
                                          nb && strcmp(nb, "loopback") == 0 ? GLF_MULTI_LOOPBACK : GLF_MULTI_RCCL, 2);
        int fstatus = out96 ? 0 : 5;
        if (glf_write_pfm_rgb("results/input.pfm", in96, (unsigned)width, (unsigned)height) != 0) fstatus = fstatus ? fstatus : 4;
        if (out96 && glf_write_pfm_rgb("results/output.pfm", out96, (unsigned)width, (unsigned)height) != 0) fstatus = fstatus ? fstatus : 4;
        if (out96 && g_nplanes && planes_write((unsigned)width, (unsigned)height, "float colour") != 0) fstatus = fstatus ? fstatus : 4;
        printf("Total computation time: %fs\n", wtime() - start_time);
        free_rows16(in96, height);
        free_rows16(out96, height);
        FinalizeProgram();
        return fstatus;
    }
    if (opt_has("-color")) { /* python/image_processing.py:410-432 */
        unsigned cw = 0, ch = 0;
        png_bytep *in_rgb = NULL;
        png_bytep *out_rgb = ColorComputation(filename, &cw, &ch, &in_rgb);
        int cstatus = out_rgb ? 0 : 5;
        if (in_rgb && glf_write_png_rgb("results/input.png", in_rgb, cw, ch) != 0) cstatus = cstatus ? cstatus : 4;
        if (out_rgb && glf_write_png_rgb("results/output.png", out_rgb, cw, ch) != 0) cstatus = cstatus ? cstatus : 4;
        if (out_rgb && g_nplanes && planes_write(cw, ch, "colour") != 0) cstatus = cstatus ? cstatus : 4;
        if (!in_rgb) {
            fprintf(stderr, "Could not read %s as an 8-bit gray / RGB / RGBA PNG\n", filename);
            cstatus = 1;
        }
        printf("Total computation time: %fs\n", wtime() - start_time);
        free_rows(in_rgb, (int)ch);
        free_rows(out_rgb, (int)ch);
        FinalizeProgram();
        return cstatus;
    }
    if (read_png(filename, &img_bytes, &width, &height) != 0) { /* ReadAndBcastImage :291; status checked here */
        fprintf(stderr, "Could not read %s as an 8-bit gray / RGB / RGBA PNG\n", filename);
        FinalizeProgram();
        return 1;
    }
    printf("Read image %s of size %dx%d => %d pixels\n", filename, width, height, width * height);

    int status = 0;
    if (opt_has("-no_approx")) { /* :294-297 */
        output_img = EntireComputation(img_bytes, (unsigned)width, (unsigned)height);
    } else if (ngpu > 0) {
        output_img = MultiComputation(img_bytes, (unsigned)width, (unsigned)height, ngpu,
                                      nb && strcmp(nb, "loopback") == 0 ? GLF_MULTI_LOOPBACK : GLF_MULTI_RCCL);
    } else if (opt_has("-fused")) {
        output_img = FusedComputation(img_bytes, (unsigned)width, (unsigned)height);
    } else {
        output_img = ApproximationComputation(img_bytes, (unsigned)width, (unsigned)height); /* :300 */
    }

    if (write_png("results/input.png", img_bytes, (unsigned)width, (unsigned)height) != 0) status = status ? status : 4; /* :306 */
    if (output_img) {
        if (write_png("results/output.png", output_img, (unsigned)width, (unsigned)height) != 0) status = status ? status : 4; /* :309 */
    } else if (!status) {
        status = 5;
    }
    if (output_img && opt_has("-dump_residual")) { /* residuals(y, z), python/image_processing.py:378-380 */
        int lo = 255, hi = 0;
        for (int r = 0; r < height; ++r)
            for (int c = 0; c < width; ++c) {
                const int d = abs((int)img_bytes[r][c] - (int)output_img[r][c]);
                lo = d < lo ? d : lo;
                hi = d > hi ? d : hi;
            }
        png_bytep *res = (png_bytep *)malloc(sizeof(png_bytep) * (size_t)height);
        for (int r = 0; res && r < height; ++r) {
            res[r] = (png_bytep)malloc((size_t)width);
            for (int c = 0; res[r] && c < width; ++c) {
                const int d = abs((int)img_bytes[r][c] - (int)output_img[r][c]);
                res[r][c] = (png_byte)(hi > lo ? ((d - lo) * 255 + (hi - lo) / 2) / (hi - lo) : 0);
            }
        }
        if (res && write_png("results/residuals.png", res, (unsigned)width, (unsigned)height) != 0) status = status ? status : 4;
        free_rows(res, height);
        printf("Residual |input - output|: min %d, max %d grey levels\n", lo, hi);
    }
    printf("Total computation time: %fs\n", wtime() - start_time); /* :314 */

    free_rows(img_bytes, height);
    free_rows(output_img, height);
    FinalizeProgram();
    return status;
}
