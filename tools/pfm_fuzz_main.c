/* pfm_fuzz_main.c -- the PFM codec under the address and undefined-behaviour sanitizers (make pfm_check). A stand-alone program: it
 * links host/pfm_codec.c directly and runs on a CPU. It feeds glf_read_pfm and glf_read_pfm_rgb the malformed files the readers must
 * refuse, every prefix of a valid file in both byte orders, and a write / read round trip; the sanitizers report any read past the
 * file's buffer. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "glf.h"

static char path[64];
static int failures = 0;

static void put(const void *data, size_t len)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(data, 1, len, f) != len) {
        perror(path);
        exit(2);
    }
    fclose(f);
}

static void free_rows(float **rows, int h)
{
    if (!rows) return;
    for (int y = 0; y < h; ++y) free(rows[y]);
    free(rows);
}

static int colour = 0; /* the reader under test: glf_read_pfm or glf_read_pfm_rgb */

/* reads the file at `path`: expect = -1 (refused, rows NULL) or 0 */
static void expect_read(const char *what, int expect)
{
    float **rows = NULL;
    int w = -7, h = -7;
    const int rc = colour ? glf_read_pfm_rgb(path, &rows, &w, &h) : glf_read_pfm(path, &rows, &w, &h);
    if (rc != expect || (rc != 0 && rows != NULL)) {
        printf("FAIL %s: rc %d (expected %d)\n", what, rc, expect);
        ++failures;
    }
    if (rc == 0) free_rows(rows, h);
}

static void text_case(const char *what, const char *text, size_t pad_floats, int expect)
{
    uint8_t buf[512];
    const size_t n = strlen(text);
    memcpy(buf, text, n);
    memset(buf + n, 0, 4 * pad_floats);
    put(buf, n + 4 * pad_floats);
    expect_read(what, expect);
}

int main(void)
{
    snprintf(path, sizeof path, "/tmp/pfm_fuzz_%ld.pfm", (long)getpid());
    int cases = 0;

    /* malformed files */
    text_case("colour PF", "PF\n3 2\n-1.0\n", 18, -1), ++cases;
    text_case("truncated data", "Pf\n3 2\n-1.0\n", 5, -1), ++cases;
    text_case("zero width", "Pf\n0 5\n-1.0\n", 6, -1), ++cases;
    text_case("zero height", "Pf\n5 0\n-1.0\n", 6, -1), ++cases;
    text_case("width overflows int", "Pf\n99999999999 5\n-1.0\n", 6, -1), ++cases;
    text_case("size overflows", "Pf\n2147483647 2147483647\n-1.0\n", 6, -1), ++cases;
    text_case("negative width", "Pf\n-3 2\n-1.0\n", 6, -1), ++cases;
    text_case("missing scale line", "Pf\n3 2\n", 6, -1), ++cases;
    text_case("zero scale", "Pf\n3 2\n0\n", 6, -1), ++cases;
    text_case("scale not a number", "Pf\n3 2\nabc\n", 6, -1), ++cases;
    text_case("no whitespace after magic", "Pf3 2\n-1.0\n", 6, -1), ++cases;
    text_case("long token", "Pf\n3 2\n-1.00000000000000000000000000000000000000000000000000000000000000000000000000\n", 6, -1), ++cases;
    put("", 0);
    expect_read("empty file", -1), ++cases;
    text_case("any whitespace", "Pf \t\r\n3\n\n2 \t-1.0\n", 6, 0), ++cases;
    text_case("big-endian", "Pf\n3 2\n1.0\n", 6, 0), ++cases;

    /* every prefix of a valid file, both byte orders: only the whole file reads */
    for (int big = 0; big < 2; ++big) {
        uint8_t file[128];
        const char *hdr = big ? "Pf\n3 2\n1.0\n" : "Pf\n3 2\n-1.0\n";
        const size_t hn = strlen(hdr), total = hn + 24;
        memcpy(file, hdr, hn);
        for (size_t i = 0; i < 24; ++i) file[hn + i] = (uint8_t)(17 * i + 3);
        for (size_t n = 0; n <= total; ++n) {
            put(file, n);
            expect_read(big ? "prefix (big-endian)" : "prefix (little-endian)", n == total ? 0 : -1);
            ++cases;
        }
    }

    /* write then read, bit for bit */
    {
        enum { W = 37, H = 19 };
        float *rows[H], store[H][W];
        for (int y = 0; y < H; ++y) {
            rows[y] = store[y];
            for (int x = 0; x < W; ++x) {
                const uint32_t bits = (uint32_t)(y * W + x) * 2654435761u; /* (any bit pattern, NaN payloads included) */
                memcpy(&store[y][x], &bits, 4);
            }
        }
        float **back = NULL;
        int w = 0, h = 0;
        if (glf_write_pfm(path, rows, W, H) != 0 || glf_read_pfm(path, &back, &w, &h) != 0 || w != W || h != H) {
            printf("FAIL round trip\n");
            ++failures;
        } else
            for (int y = 0; y < H; ++y)
                if (memcmp(back[y], store[y], sizeof store[y]) != 0) {
                    printf("FAIL round trip row %d\n", y);
                    ++failures;
                }
        free_rows(back, h);
        ++cases;
        float **null_rows = NULL;
        if (glf_read_pfm(NULL, &null_rows, &w, &h) != -1 || glf_write_pfm(path, NULL, 3, 2) != -1 || glf_write_pfm(path, rows, 0, 2) != -1) {
            printf("FAIL null arguments\n");
            ++failures;
        }
        ++cases;
    }

    /* the colour reader: the same malformed headers under its magic, the grey magic, every prefix, the round trip */
    colour = 1;
    text_case("colour: grey Pf", "Pf\n3 2\n-1.0\n", 18, -1), ++cases;
    text_case("colour: grey-sized data", "PF\n3 2\n-1.0\n", 6, -1), ++cases;
    text_case("colour: one float short", "PF\n3 2\n-1.0\n", 17, -1), ++cases;
    text_case("colour: zero width", "PF\n0 5\n-1.0\n", 18, -1), ++cases;
    text_case("colour: zero height", "PF\n5 0\n-1.0\n", 18, -1), ++cases;
    text_case("colour: width overflows int", "PF\n99999999999 5\n-1.0\n", 18, -1), ++cases;
    text_case("colour: size overflows", "PF\n2147483647 2147483647\n-1.0\n", 18, -1), ++cases;
    text_case("colour: 3 x size overflows", "PF\n1431655766 3221225472\n-1.0\n", 18, -1), ++cases;
    text_case("colour: negative width", "PF\n-3 2\n-1.0\n", 18, -1), ++cases;
    text_case("colour: missing scale line", "PF\n3 2\n", 18, -1), ++cases;
    text_case("colour: zero scale", "PF\n3 2\n0\n", 18, -1), ++cases;
    text_case("colour: scale not a number", "PF\n3 2\nabc\n", 18, -1), ++cases;
    text_case("colour: no whitespace after magic", "PF3 2\n-1.0\n", 18, -1), ++cases;
    text_case("colour: long token", "PF\n3 2\n-1.00000000000000000000000000000000000000000000000000000000000000000000000000\n", 18, -1), ++cases;
    put("", 0);
    expect_read("colour: empty file", -1), ++cases;
    text_case("colour: any whitespace", "PF \t\r\n3\n\n2 \t-1.0\n", 18, 0), ++cases;
    text_case("colour: big-endian", "PF\n3 2\n1.0\n", 18, 0), ++cases;
    for (int big = 0; big < 2; ++big) {
        uint8_t file[128];
        const char *hdr = big ? "PF\n3 2\n1.0\n" : "PF\n3 2\n-1.0\n";
        const size_t hn = strlen(hdr), total = hn + 72;
        memcpy(file, hdr, hn);
        for (size_t i = 0; i < 72; ++i) file[hn + i] = (uint8_t)(17 * i + 3);
        for (size_t n = 0; n <= total; ++n) {
            put(file, n);
            expect_read(big ? "colour: prefix (big-endian)" : "colour: prefix (little-endian)", n == total ? 0 : -1);
            ++cases;
        }
    }
    {
        enum { W = 37, H = 19 };
        static float store[H][3 * W];
        float *rows[H];
        for (int y = 0; y < H; ++y) {
            rows[y] = store[y];
            for (int x = 0; x < 3 * W; ++x) {
                const uint32_t bits = (uint32_t)(y * 3 * W + x) * 2654435761u;
                memcpy(&store[y][x], &bits, 4);
            }
        }
        float **back = NULL;
        int w = 0, h = 0;
        if (glf_write_pfm_rgb(path, rows, W, H) != 0 || glf_read_pfm_rgb(path, &back, &w, &h) != 0 || w != W || h != H) {
            printf("FAIL colour round trip\n");
            ++failures;
        } else
            for (int y = 0; y < H; ++y)
                if (memcmp(back[y], store[y], sizeof store[y]) != 0) {
                    printf("FAIL colour round trip row %d\n", y);
                    ++failures;
                }
        free_rows(back, h);
        ++cases;
        float **grey = NULL; /* the colour file under the grey reader */
        if (glf_read_pfm(path, &grey, &w, &h) != -1 || grey != NULL) {
            printf("FAIL colour file under the grey reader\n");
            ++failures;
        }
        ++cases;
        float **null_rows = NULL;
        if (glf_read_pfm_rgb(NULL, &null_rows, &w, &h) != -1 || glf_write_pfm_rgb(path, NULL, 3, 2) != -1 ||
            glf_write_pfm_rgb(path, rows, 0, 2) != -1) {
            printf("FAIL colour null arguments\n");
            ++failures;
        }
        ++cases;
    }
    remove(path);
    printf("pfm_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
