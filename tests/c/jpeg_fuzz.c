/* Stand-alone driver for csrc_host/xmc_jpeg.c under -fsanitize=address,undefined (tests/test_jpeg.py compiles both and
 * runs this as a subprocess; no Python, no preload, no GPU).  For every file named on the command line:
 *   1. the file truncated at each byte offset,
 *   2. 2,000 seeded single- and multi-byte corruptions of it
 * go through xmc_jpeg_info and, where that succeeds, xmc_jpeg_coefficients with buffers of EXACTLY the sizes it stated, so a
 * write past either is a sanitizer report.  Every call must return; the program exits 0 when all did. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int xmc_jpeg_info(const void* data, int64_t n, int32_t* info);
int xmc_jpeg_coefficients(const void* data, int64_t n, int16_t* coef, int64_t coef_bytes, uint16_t* qt, int64_t qt_bytes);

static uint64_t rng_state;
static uint32_t rng(void) {                                   /* xorshift64* */
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 2685821237ULL) >> 32);
}

static long calls, accepted;

static void feed(const uint8_t* data, int64_t n) {
    /* an exact-size heap copy: a read past the end of the input is a report too */
    uint8_t* copy = (uint8_t*)malloc(n ? (size_t)n : 1);
    memcpy(copy, data, (size_t)n);
    int32_t info[16];
    ++calls;
    if (xmc_jpeg_info(copy, n, info) == 0) {
        int16_t* coef = (int16_t*)malloc((size_t)info[8] ? (size_t)info[8] : 1);
        uint16_t* qt = (uint16_t*)malloc((size_t)info[9] ? (size_t)info[9] : 1);
        if (xmc_jpeg_coefficients(copy, n, coef, info[8], qt, info[9]) == 0) ++accepted;
        free(coef);
        free(qt);
    }
    free(copy);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        fseek(f, 0, SEEK_END);
        long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = (uint8_t*)malloc((size_t)n);
        if (fread(data, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        long before = accepted;
        feed(data, n);
        if (accepted != before + 1 && !strstr(argv[a], "cmyk")) {
            fprintf(stderr, "%s: the intact file was not decoded\n", argv[a]);
            return 3;
        }
        for (long cut = 0; cut < n; ++cut) feed(data, cut);
        uint8_t* bad = (uint8_t*)malloc((size_t)n);
        rng_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t)a;
        for (int trial = 0; trial < 2000; ++trial) {
            memcpy(bad, data, (size_t)n);
            int hits = (trial & 1) ? 1 + (int)(rng() % 4) : 1;
            for (int h = 0; h < hits; ++h) {
                uint32_t pos = rng() % (uint32_t)n, mode = rng() % 3;
                bad[pos] = mode == 0 ? (uint8_t)rng() : mode == 1 ? 0xFF : (uint8_t)(bad[pos] ^ (1u << (rng() % 8)));
            }
            feed(bad, n);
        }
        free(bad);
        free(data);
    }
    printf("%ld calls, %ld accepted\n", calls, accepted);
    return 0;
}
