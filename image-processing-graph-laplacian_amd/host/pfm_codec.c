/* pfm_codec.c -- the Portable Float Map, greyscale and colour: the float image files of the host program (a PNG cannot hold a float).
 *
 * Layout: the header "Pf\n<width> <height>\n<scale>\n" -- three tokens after the magic, any whitespace between them, exactly one
 * whitespace byte after the scale -- then width * height raw IEEE floats, BOTTOM row first. scale < 0: the floats are little-endian,
 * scale > 0: big-endian (its magnitude is a display hint and is ignored). "PF" is the three-channel variant: the same header, rows of
 * 3 * width floats (R G B interleaved). Each reader takes its own magic only: glf_read_pfm refuses "PF", glf_read_pfm_rgb refuses "Pf".
 *
 * The reader holds the whole file in one buffer and never reads past it: every header byte is fetched through a bounds check, and the
 * pixel count is compared with the bytes that remain by division, so a size that overflows cannot pass.
 */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "glf.h"

static int pfm_space(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

/* skips whitespace (at least `need` bytes of it), then copies one token of at most cap - 1 bytes; 0 / -1 */
static int pfm_token(const uint8_t *buf, size_t len, size_t *pos, size_t need, char *tok, size_t cap)
{
    size_t i = *pos, skipped = 0, n = 0;
    while (i < len && pfm_space(buf[i])) ++i, ++skipped;
    if (skipped < need) return -1;
    while (i < len && !pfm_space(buf[i])) {
        if (n + 1 >= cap) return -1;
        tok[n++] = (char)buf[i++];
    }
    if (n == 0) return -1;
    tok[n] = 0;
    *pos = i;
    return 0;
}

/* a positive decimal integer that fits an int; 0 / -1 */
static int pfm_dim(const char *tok, int *out)
{
    long long v = 0;
    if (!*tok) return -1;
    for (const char *q = tok; *q; ++q) {
        if (*q < '0' || *q > '9') return -1;
        v = v * 10 + (*q - '0');
        if (v > INT_MAX) return -1;
    }
    if (v <= 0) return -1;
    *out = (int)v;
    return 0;
}

/* the parse of a file image in memory with nch (1: "Pf", 3: "PF") floats per pixel: rows (malloc'd, top first, nch * width floats
 * each) or -1 */
static int pfm_parse(const uint8_t *buf, size_t len, int nch, float ***rows_out, int *width, int *height)
{
    if (!buf || !rows_out || !width || !height) return -1;
    *rows_out = NULL;
    if (len < 2 || buf[0] != 'P' || buf[1] != (nch == 3 ? 'F' : 'f')) return -1; /* (the other variant's magic included) */
    size_t pos = 2;
    char tw[16], th[16], ts[64];
    int w = 0, h = 0;
    if (pfm_token(buf, len, &pos, 1, tw, sizeof tw) != 0 || pfm_dim(tw, &w) != 0) return -1;
    if (pfm_token(buf, len, &pos, 1, th, sizeof th) != 0 || pfm_dim(th, &h) != 0) return -1;
    if (pfm_token(buf, len, &pos, 1, ts, sizeof ts) != 0) return -1;
    char *end = NULL;
    const double scale = strtod(ts, &end);
    if (end == ts || *end != 0 || !isfinite(scale) || scale == 0.0) return -1;
    if (pos >= len || !pfm_space(buf[pos])) return -1; /* one whitespace byte, then the data */
    ++pos;
    const size_t remain = len - pos;
    if ((size_t)w > remain / sizeof(float) / (size_t)nch / (size_t)h) return -1; /* short file (or a size that overflows) */
    const size_t rowf = (size_t)nch * (size_t)w;                                 /* floats per row: fits, it passed the check */
    const int big = scale > 0.0;
    float **rows = (float **)calloc((size_t)h, sizeof(float *));
    if (!rows) return -1;
    for (int y = 0; y < h; ++y) {
        rows[y] = (float *)malloc(sizeof(float) * rowf);
        if (!rows[y]) {
            for (int q = 0; q < y; ++q) free(rows[q]);
            free(rows);
            return -1;
        }
        const uint8_t *src = buf + pos + sizeof(float) * rowf * (size_t)(h - 1 - y); /* (the file's first row is the bottom one) */
        for (size_t x = 0; x < rowf; ++x) {
            const uint8_t *b = src + 4 * x;
            const uint32_t v = big ? ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]
                                   : ((uint32_t)b[3] << 24) | ((uint32_t)b[2] << 16) | ((uint32_t)b[1] << 8) | b[0];
            memcpy(&rows[y][x], &v, sizeof v);
        }
    }
    *rows_out = rows;
    *width = w;
    *height = h;
    return 0;
}

static int pfm_read(const char *filename, int nch, float ***rows, int *width, int *height)
{
    if (!filename || !rows || !width || !height) return -1;
    *rows = NULL;
    FILE *f = fopen(filename, "rb");
    if (!f) {
        fprintf(stderr, "Could not open file %s\n", filename);
        return -1;
    }
    int rc = -1;
    uint8_t *buf = NULL;
    if (fseek(f, 0, SEEK_END) != 0) goto done;
    const long flen = ftell(f);
    if (flen <= 0 || fseek(f, 0, SEEK_SET) != 0) goto done;
    buf = (uint8_t *)malloc((size_t)flen);
    if (!buf || fread(buf, 1, (size_t)flen, f) != (size_t)flen) goto done;
    rc = pfm_parse(buf, (size_t)flen, nch, rows, width, height);
done:
    free(buf);
    fclose(f);
    return rc;
}

int glf_read_pfm(const char *filename, float ***rows, int *width, int *height) { return pfm_read(filename, 1, rows, width, height); }

int glf_read_pfm_rgb(const char *filename, float ***rows, int *width, int *height) { return pfm_read(filename, 3, rows, width, height); }

static int pfm_write(const char *filename, unsigned nch, float **rows, unsigned width, unsigned height)
{
    if (!filename || !rows || width == 0 || height == 0 || width > INT_MAX / nch || height > INT_MAX) return -1;
    const char *magic = nch == 3 ? "PF" : "Pf";
    const size_t rowf = (size_t)nch * width;
    FILE *f = fopen(filename, "wb");
    if (!f) {
        fprintf(stderr, "Could not open file %s\n", filename);
        return -1;
    }
    int rc = -1;
    uint8_t *line = (uint8_t *)malloc(4 * rowf);
    if (!line) goto done;
    if (fprintf(f, "%s\n%u %u\n-1.0\n", magic, width, height) < 0) goto done;
    for (unsigned y = height; y-- > 0;) { /* bottom row first */
        if (!rows[y]) goto done;
        for (size_t x = 0; x < rowf; ++x) {
            uint32_t v;
            memcpy(&v, &rows[y][x], sizeof v);
            line[4 * x] = (uint8_t)v;
            line[4 * x + 1] = (uint8_t)(v >> 8);
            line[4 * x + 2] = (uint8_t)(v >> 16);
            line[4 * x + 3] = (uint8_t)(v >> 24);
        }
        if (fwrite(line, 4, rowf, f) != rowf) goto done;
    }
    rc = 0;
done:
    free(line);
    if (fclose(f) != 0) rc = -1;
    return rc;
}

int glf_write_pfm(const char *filename, float **rows, unsigned width, unsigned height) { return pfm_write(filename, 1, rows, width, height); }

int glf_write_pfm_rgb(const char *filename, float **rows, unsigned width, unsigned height) { return pfm_write(filename, 3, rows, width, height); }
