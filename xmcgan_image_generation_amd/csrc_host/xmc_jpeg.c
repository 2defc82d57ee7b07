/* JPEG entropy decoder (ITU-T T.81): the serial half of a JPEG decode, on the host.  It parses the marker segments and decodes
 * the Huffman-coded scans of 8-bit baseline / extended sequential / progressive files into QUANTISED coefficients (int16,
 * natural order, [block_row][block_col][64] per component, padded to whole MCUs) plus the quantisation tables.  No pixel
 * arithmetic happens here: dequantisation, the inverse DCT, chroma upsampling and the colour conversion are the device stage
 * (csrc_codec/jpeg.hip) or its NumPy statement (libml/jpeg.py).
 *
 * Held to the bar of xmc_inflate.c: every read is bounds-checked against the input, every write against the coefficient
 * buffer, arithmetic that could overflow is range-checked first, and damaged input ends in an error code in bounded time.
 * What the decoder does not support is refused with its own code, never guessed at. */
#include <stdint.h>
#include <string.h>

#define XMC_JPEG_E_MALFORMED   (-1)   /* not a JPEG, or a marker segment that contradicts the standard */
#define XMC_JPEG_E_TRUNCATED   (-2)   /* the data ends before the image does (no EOI, or entropy bits past the end) */
#define XMC_JPEG_E_HUFFMAN     (-3)   /* a bit pattern that is no code of the table in use, or a scan that runs into a marker */
#define XMC_JPEG_E_RUN         (-4)   /* a zero run or a band that passes coefficient 63 / Se */
#define XMC_JPEG_E_RESTART     (-5)   /* the restart marker due is missing or is the wrong one */
#define XMC_JPEG_E_TABLE       (-6)   /* a table index out of range, or a table used before it is defined */
#define XMC_JPEG_E_BUFFER      (-7)   /* the caller's buffer is smaller than xmc_jpeg_info said */
#define XMC_JPEG_E_RANGE       (-8)   /* a coefficient that does not fit int16 */
#define XMC_JPEG_E_SCANS       (-9)   /* more than XMC_JPEG_MAX_SCANS scans: every scan may walk every block of the image */
#define XMC_JPEG_E_ARITHMETIC  (-10)  /* arithmetic coding (SOF9-11, 13-15, DAC) */
#define XMC_JPEG_E_PRECISION   (-11)  /* sample precision other than 8 bits */
#define XMC_JPEG_E_PROCESS     (-12)  /* lossless or hierarchical processes (SOF3, 5-7) */
#define XMC_JPEG_E_COMPONENTS  (-13)  /* component count other than 1 or 3 (CMYK / YCCK) */
#define XMC_JPEG_E_SAMPLING    (-14)  /* sampling other than luma 1x1 / 2x1 / 2x2 with 1x1 chroma */
#define XMC_JPEG_E_SIZE        (-15)  /* a side above 16384 or more than 2^26 pixels */

#define XMC_JPEG_MAX_SIDE 16384
#define XMC_JPEG_MAX_PIXELS (1 << 26)
#define XMC_JPEG_INFO_WORDS 16
/* what bounds the work per input byte: a legitimate progressive file has about ten scans (libjpeg's default script), at most
 * a few dozen; without a cap a small file declared at the size cap could ask for thousands of passes over 10^6 blocks */
#define XMC_JPEG_MAX_SCANS 256

static const uint8_t ZIGZAG[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

typedef struct {
    int defined;
    uint16_t fast[512];          /* 9-bit prefix -> (length << 8) | symbol, 0: longer than 9 bits or no code */
    int32_t maxcode[18];         /* largest code of each length, -1: none */
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
} huff_t;

typedef struct {
    int id, h, v, tq;
    int bw, bh;                  /* blocks per row / column of the padded plane */
    int cw, ch;                  /* blocks that hold samples (a non-interleaved scan codes only these) */
    int64_t off;                 /* first int16 of the plane in the coefficient buffer */
    int dc_seen;
} comp_t;

typedef struct {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;
    int cnt;
    int64_t fake;                /* zero bytes fed after a marker or the end of the data */
    int marker;
} bits_t;

typedef struct {
    int width, height, ncomp, process, hmax, vmax, mcus_x, mcus_y, have_sof;
    comp_t comp[3];
    uint16_t qt[4][64];
    int qt_defined[4];
    huff_t dc[4], ac[4];
    int restart_interval;
    int64_t coef_count;
} jpeg_t;

static void bits_fill(bits_t* b) {
    while (b->cnt <= 56) {
        int byte = 0;
        if (b->marker || b->p >= b->end) {
            b->fake++;
        } else {
            byte = *b->p;
            if (byte == 0xFF) {
                if (b->p + 1 >= b->end) {
                    b->p = b->end;
                    byte = 0;
                    b->fake++;
                } else if (b->p[1] == 0) {
                    b->p += 2;
                } else if (b->p[1] == 0xFF) {
                    b->p++;                 /* fill byte in front of a marker */
                    continue;
                } else {
                    b->marker = b->p[1];    /* p stays on the marker */
                    byte = 0;
                    b->fake++;
                }
            } else {
                b->p++;
            }
        }
        b->buf |= (uint64_t)byte << (56 - b->cnt);
        b->cnt += 8;
    }
}

/* bits of the padding have been consumed: the scan ran past its data */
static inline int bits_overrun(const bits_t* b) { return (int64_t)b->cnt < b->fake * 8; }

static inline void bits_need(bits_t* b) {
    if (b->cnt < 32) bits_fill(b);
}

static inline int bits_get(bits_t* b, int n) {          /* n in [0, 16], after bits_need */
    if (n == 0) return 0;
    int v = (int)(b->buf >> (64 - n));
    b->buf <<= n;
    b->cnt -= n;
    return v;
}

static inline int huff_decode(bits_t* b, const huff_t* h) {     /* symbol, or -1 */
    int look = (int)(b->buf >> 55);
    int e = h->fast[look];
    if (e) {
        int len = e >> 8;
        b->buf <<= len;
        b->cnt -= len;
        return e & 0xFF;
    }
    for (int len = 10; len <= 16; ++len) {
        int32_t code = (int32_t)(b->buf >> (64 - len));
        if (code <= h->maxcode[len] && code >= h->mincode[len]) {
            b->buf <<= len;
            b->cnt -= len;
            return h->vals[h->valptr[len] + code - h->mincode[len]];
        }
    }
    return -1;
}

static inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

static int build_huffman(huff_t* h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    memset(h, 0, sizeof(*h));
    memcpy(h->vals, vals, (size_t)nvals);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        h->valptr[len] = k;
        h->mincode[len] = code;
        int c = counts[len - 1];
        if (code + c > (1 << len)) return XMC_JPEG_E_MALFORMED;         /* more codes than the length has */
        for (int i = 0; i < c; ++i, ++k, ++code) {
            if (len <= 9) {
                int lo = code << (9 - len), n = 1 << (9 - len);
                for (int j = 0; j < n; ++j) h->fast[lo + j] = (uint16_t)((len << 8) | vals[k]);
            }
        }
        h->maxcode[len] = c ? code - 1 : -1;
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    h->defined = 1;
    return 0;
}

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

static int parse_sof(jpeg_t* j, const uint8_t* s, int len, int marker) {
    if (j->have_sof) return XMC_JPEG_E_MALFORMED;
    if (len < 6) return XMC_JPEG_E_MALFORMED;
    int prec = s[0], height = be16(s + 1), width = be16(s + 3), nc = s[5];
    if (prec != 8) return (prec == 12 || prec == 16) ? XMC_JPEG_E_PRECISION : XMC_JPEG_E_MALFORMED;
    if (nc != 1 && nc != 3) return (nc == 4 || nc == 2) ? XMC_JPEG_E_COMPONENTS : XMC_JPEG_E_MALFORMED;
    if (len != 6 + 3 * nc) return XMC_JPEG_E_MALFORMED;
    if (width == 0 || height == 0) return XMC_JPEG_E_MALFORMED;          /* (height 0 = DNL: not supported, not guessed) */
    if (width > XMC_JPEG_MAX_SIDE || height > XMC_JPEG_MAX_SIDE || (int64_t)width * height > XMC_JPEG_MAX_PIXELS)
        return XMC_JPEG_E_SIZE;
    j->width = width, j->height = height, j->ncomp = nc;
    j->process = marker == 0xC0 ? 0 : marker == 0xC1 ? 1 : 2;
    for (int c = 0; c < nc; ++c) {
        comp_t* k = &j->comp[c];
        k->id = s[6 + 3 * c];
        k->h = s[7 + 3 * c] >> 4, k->v = s[7 + 3 * c] & 15;
        k->tq = s[8 + 3 * c];
        if (k->tq > 3) return XMC_JPEG_E_TABLE;
        if (k->h < 1 || k->h > 4 || k->v < 1 || k->v > 4) return XMC_JPEG_E_MALFORMED;
        for (int d = 0; d < c; ++d)
            if (j->comp[d].id == k->id) return XMC_JPEG_E_MALFORMED;
    }
    if (nc == 1) {
        j->comp[0].h = j->comp[0].v = 1;           /* one component is never interleaved: its factors mean nothing (A.2.2) */
    } else {
        int h = j->comp[0].h, v = j->comp[0].v;
        if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return XMC_JPEG_E_SAMPLING;
        for (int c = 1; c < 3; ++c)
            if (j->comp[c].h != 1 || j->comp[c].v != 1) return XMC_JPEG_E_SAMPLING;
    }
    j->hmax = j->comp[0].h, j->vmax = j->comp[0].v;
    j->mcus_x = (width + 8 * j->hmax - 1) / (8 * j->hmax);
    j->mcus_y = (height + 8 * j->vmax - 1) / (8 * j->vmax);
    int64_t off = 0;
    for (int c = 0; c < nc; ++c) {
        comp_t* k = &j->comp[c];
        k->bw = j->mcus_x * k->h, k->bh = j->mcus_y * k->v;
        int sw = (width * k->h + j->hmax - 1) / j->hmax, sh = (height * k->v + j->vmax - 1) / j->vmax;
        k->cw = (sw + 7) / 8, k->ch = (sh + 7) / 8;
        k->off = off;
        off += (int64_t)k->bw * k->bh * 64;
    }
    j->coef_count = off;
    j->have_sof = 1;
    return 0;
}

static int parse_dqt(jpeg_t* j, const uint8_t* s, int len) {
    while (len > 0) {
        int pq = s[0] >> 4, tq = s[0] & 15;
        if (pq > 1) return XMC_JPEG_E_MALFORMED;
        if (tq > 3) return XMC_JPEG_E_TABLE;
        int need = 1 + 64 * (pq + 1);
        if (len < need) return XMC_JPEG_E_MALFORMED;
        for (int i = 0; i < 64; ++i)
            j->qt[tq][ZIGZAG[i]] = (uint16_t)(pq ? be16(s + 1 + 2 * i) : s[1 + i]);
        j->qt_defined[tq] = 1;
        s += need, len -= need;
    }
    return 0;
}

static int parse_dht(jpeg_t* j, const uint8_t* s, int len) {
    while (len > 0) {
        if (len < 17) return XMC_JPEG_E_MALFORMED;
        int tc = s[0] >> 4, th = s[0] & 15;
        if (tc > 1) return XMC_JPEG_E_MALFORMED;
        if (th > 3) return XMC_JPEG_E_TABLE;
        int n = 0;
        for (int i = 0; i < 16; ++i) n += s[1 + i];
        if (n > 256 || len < 17 + n) return XMC_JPEG_E_MALFORMED;
        int rc = build_huffman(tc ? &j->ac[th] : &j->dc[th], s + 1, s + 17, n);
        if (rc) return rc;
        s += 17 + n, len -= 17 + n;
    }
    return 0;
}

typedef struct {
    int ns, ss, se, ah, al;
    comp_t* comp[3];
    const huff_t* dc[3];
    const huff_t* ac[3];
    int pred[3];
    int eobrun;
} scan_t;

static inline int store_coef(int16_t* dst, int v) {
    if (v < -32768 || v > 32767) return XMC_JPEG_E_RANGE;
    *dst = (int16_t)v;
    return 0;
}

/* one block of a sequential scan */
static int block_sequential(bits_t* b, scan_t* sc, int ci, int16_t* blk) {
    bits_need(b);
    int s = huff_decode(b, sc->dc[ci]);
    if (s < 0 || s > 11) return XMC_JPEG_E_HUFFMAN;
    int diff = s ? extend(bits_get(b, s), s) : 0;
    sc->pred[ci] += diff;
    int rc = store_coef(&blk[0], sc->pred[ci]);
    if (rc) return rc;
    const huff_t* ac = sc->ac[ci];
    for (int k = 1; k < 64;) {
        bits_need(b);
        int rs = huff_decode(b, ac);
        if (rs < 0) return XMC_JPEG_E_HUFFMAN;
        int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return XMC_JPEG_E_RUN;
            blk[ZIGZAG[k]] = (int16_t)extend(bits_get(b, s), s);      /* s <= 15: fits int16 */
            ++k;
        } else if (r == 15) {
            k += 16;
        } else {
            break;
        }
    }
    return 0;
}

static int block_dc_first(bits_t* b, scan_t* sc, int ci, int16_t* blk) {
    bits_need(b);
    int s = huff_decode(b, sc->dc[ci]);
    if (s < 0 || s > 11) return XMC_JPEG_E_HUFFMAN;
    int diff = s ? extend(bits_get(b, s), s) : 0;
    sc->pred[ci] += diff;
    if (sc->pred[ci] < -32768 || sc->pred[ci] > 32767) return XMC_JPEG_E_RANGE;
    return store_coef(&blk[0], sc->pred[ci] * (1 << sc->al));
}

static int block_dc_refine(bits_t* b, scan_t* sc, int16_t* blk) {
    bits_need(b);
    if (bits_get(b, 1)) blk[0] = (int16_t)(blk[0] | (1 << sc->al));
    return 0;
}

static int block_ac_first(bits_t* b, scan_t* sc, int16_t* blk) {
    if (sc->eobrun > 0) {
        sc->eobrun--;
        return 0;
    }
    const huff_t* ac = sc->ac[0];
    for (int k = sc->ss; k <= sc->se; ++k) {
        bits_need(b);
        int rs = huff_decode(b, ac);
        if (rs < 0) return XMC_JPEG_E_HUFFMAN;
        int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > sc->se) return XMC_JPEG_E_RUN;
            int rc = store_coef(&blk[ZIGZAG[k]], extend(bits_get(b, s), s) * (1 << sc->al));
            if (rc) return rc;
        } else if (r == 15) {
            k += 15;
        } else {
            sc->eobrun = 1 << r;
            if (r) sc->eobrun += bits_get(b, r);
            sc->eobrun--;
            break;
        }
    }
    return 0;
}

/* correction bit of a coefficient that is already non-zero (G.1.2.3) */
static inline int refine_nonzero(bits_t* b, int16_t* c, int p1) {
    bits_need(b);
    if (bits_get(b, 1) && (*c & p1) == 0) return store_coef(c, *c >= 0 ? *c + p1 : *c - p1);
    return 0;
}

static int block_ac_refine(bits_t* b, scan_t* sc, int16_t* blk) {
    const int p1 = 1 << sc->al;
    const huff_t* ac = sc->ac[0];
    int k = sc->ss, rc;
    if (sc->eobrun == 0) {
        for (; k <= sc->se; ++k) {
            bits_need(b);
            int rs = huff_decode(b, ac);
            if (rs < 0) return XMC_JPEG_E_HUFFMAN;
            int r = rs >> 4, s = rs & 15, val = 0;
            if (s) {
                if (s != 1) return XMC_JPEG_E_HUFFMAN;
                val = bits_get(b, 1) ? p1 : -p1;
            } else if (r != 15) {
                sc->eobrun = 1 << r;
                if (r) sc->eobrun += bits_get(b, r);
                break;
            }
            for (; k <= sc->se; ++k) {                 /* pass non-zero history, count r zeros */
                int16_t* c = &blk[ZIGZAG[k]];
                if (*c != 0) {
                    if ((rc = refine_nonzero(b, c, p1)) != 0) return rc;
                } else if (--r < 0) {
                    break;
                }
            }
            if (val) {
                if (k > sc->se) return XMC_JPEG_E_RUN;
                blk[ZIGZAG[k]] = (int16_t)val;
            }
        }
    }
    if (sc->eobrun > 0) {
        for (; k <= sc->se; ++k) {
            int16_t* c = &blk[ZIGZAG[k]];
            if (*c != 0 && (rc = refine_nonzero(b, c, p1)) != 0) return rc;
        }
        sc->eobrun--;
    }
    return 0;
}

static int decode_block(jpeg_t* j, bits_t* b, scan_t* sc, int ci, int16_t* blk) {
    if (j->process != 2) return block_sequential(b, sc, ci, blk);
    if (sc->ss == 0) return sc->ah == 0 ? block_dc_first(b, sc, ci, blk) : block_dc_refine(b, sc, blk);
    return sc->ah == 0 ? block_ac_first(b, sc, blk) : block_ac_refine(b, sc, blk);
}

/* after an interval or a scan: drop the padding bits and stand on the next marker.  -> marker code, or an error */
static int bits_to_marker(bits_t* b) {
    if (bits_overrun(b)) return b->marker ? XMC_JPEG_E_HUFFMAN : XMC_JPEG_E_TRUNCATED;
    if (!b->marker) {
        /* whole bytes still in the bit buffer were real data: step back over them is not possible once stuffing is
         * removed, so look forward from the read position (as libjpeg does) */
        while (b->p + 1 < b->end && !(b->p[0] == 0xFF && b->p[1] != 0 && b->p[1] != 0xFF)) b->p++;
        if (b->p + 1 >= b->end) return XMC_JPEG_E_TRUNCATED;
        b->marker = b->p[1];
    }
    return b->marker;
}

static int decode_scan(jpeg_t* j, const uint8_t* hdr, int len, bits_t* b, int16_t* coef) {
    scan_t sc;
    memset(&sc, 0, sizeof(sc));
    if (len < 1) return XMC_JPEG_E_MALFORMED;
    sc.ns = hdr[0];
    if (sc.ns < 1 || sc.ns > j->ncomp || len != 4 + 2 * sc.ns) return XMC_JPEG_E_MALFORMED;
    const uint8_t* t = hdr + 1 + 2 * sc.ns;
    sc.ss = t[0], sc.se = t[1], sc.ah = t[2] >> 4, sc.al = t[2] & 15;
    if (j->process != 2) {
        if (sc.ss != 0 || sc.se != 63 || sc.ah != 0 || sc.al != 0) return XMC_JPEG_E_MALFORMED;
    } else {
        if (sc.ss > sc.se || sc.se > 63 || sc.ah > 13 || sc.al > 13) return XMC_JPEG_E_MALFORMED;
        if (sc.ss == 0 ? sc.se != 0 : sc.ns != 1) return XMC_JPEG_E_MALFORMED;
        if (sc.ah != 0 && sc.ah != sc.al + 1) return XMC_JPEG_E_MALFORMED;
    }
    for (int i = 0; i < sc.ns; ++i) {
        int id = hdr[1 + 2 * i], td = hdr[2 + 2 * i] >> 4, ta = hdr[2 + 2 * i] & 15, c;
        for (c = 0; c < j->ncomp && j->comp[c].id != id; ++c) {}
        if (c == j->ncomp) return XMC_JPEG_E_MALFORMED;
        for (int d = 0; d < i; ++d)
            if (sc.comp[d] == &j->comp[c]) return XMC_JPEG_E_MALFORMED;
        if (td > 3 || ta > 3) return XMC_JPEG_E_TABLE;
        int need_dc = sc.ss == 0 && sc.ah == 0, need_ac = j->process != 2 || sc.ss > 0;
        if ((need_dc && !j->dc[td].defined) || (need_ac && !j->ac[ta].defined)) return XMC_JPEG_E_TABLE;
        sc.comp[i] = &j->comp[c], sc.dc[i] = &j->dc[td], sc.ac[i] = &j->ac[ta];
        if (j->process != 2 && j->comp[c].dc_seen) return XMC_JPEG_E_MALFORMED;              /* a second scan of a component */
        if (sc.ss == 0 && sc.ah == 0) j->comp[c].dc_seen = 1;
        else if (j->process == 2 && !j->comp[c].dc_seen) return XMC_JPEG_E_MALFORMED;      /* a band before its DC scan */
    }
    const int inter = sc.ns > 1;
    const int nx = inter ? j->mcus_x : sc.comp[0]->cw, ny = inter ? j->mcus_y : sc.comp[0]->ch;
    int left = j->restart_interval, next_rst = 0, rc;
    for (int my = 0; my < ny; ++my) {
        for (int mx = 0; mx < nx; ++mx) {
            if (j->restart_interval && left == 0) {
                int m = bits_to_marker(b);
                if (m < 0) return m;
                if (m != 0xD0 + next_rst) return XMC_JPEG_E_RESTART;
                b->p += 2, b->marker = 0, b->fake = 0, b->buf = 0, b->cnt = 0;
                next_rst = (next_rst + 1) & 7;
                left = j->restart_interval;
                sc.pred[0] = sc.pred[1] = sc.pred[2] = 0;
                sc.eobrun = 0;
            }
            if (inter) {
                for (int i = 0; i < sc.ns; ++i) {
                    comp_t* k = sc.comp[i];
                    for (int v = 0; v < k->v; ++v)
                        for (int h = 0; h < k->h; ++h) {
                            int64_t blk = (int64_t)(my * k->v + v) * k->bw + (mx * k->h + h);
                            if ((rc = decode_block(j, b, &sc, i, coef + k->off + blk * 64)) != 0) return rc;
                        }
                }
            } else {
                comp_t* k = sc.comp[0];
                if ((rc = decode_block(j, b, &sc, 0, coef + k->off + ((int64_t)my * k->bw + mx) * 64)) != 0) return rc;
            }
            --left;
        }
        if (bits_overrun(b)) return b->marker ? XMC_JPEG_E_HUFFMAN : XMC_JPEG_E_TRUNCATED;
    }
    rc = bits_to_marker(b);
    return rc < 0 ? rc : 0;
}

/* the marker walk.  coef == NULL: stop after the frame header (xmc_jpeg_info) */
static int decode(jpeg_t* j, const uint8_t* data, int64_t n, int16_t* coef, int64_t coef_capacity) {
    memset(j, 0, sizeof(*j));
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return XMC_JPEG_E_MALFORMED;
    const uint8_t* p = data + 2;
    const uint8_t* end = data + n;
    int scans = 0;
    for (;;) {
        if (p + 2 > end) return XMC_JPEG_E_TRUNCATED;
        if (p[0] != 0xFF) return XMC_JPEG_E_MALFORMED;
        if (p[1] == 0xFF) {
            ++p;
            continue;
        }
        int m = p[1];
        p += 2;
        if (m == 0xD9) break;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0 || m == 0xD8) return XMC_JPEG_E_MALFORMED;
        if (p + 2 > end) return XMC_JPEG_E_TRUNCATED;
        int len = be16(p);
        if (len < 2) return XMC_JPEG_E_MALFORMED;
        if (len > end - p) return XMC_JPEG_E_TRUNCATED;
        const uint8_t* s = p + 2;
        p += len;
        len -= 2;
        int rc = 0;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
            rc = parse_sof(j, s, len, m);
            if (rc == 0 && coef == NULL) return 0;
            if (rc == 0 && coef_capacity < j->coef_count) return XMC_JPEG_E_BUFFER;
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            rc = XMC_JPEG_E_PROCESS;
        } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC) {
            rc = XMC_JPEG_E_ARITHMETIC;
        } else if (m == 0xC4) {
            rc = parse_dht(j, s, len);
        } else if (m == 0xDB) {
            rc = parse_dqt(j, s, len);
        } else if (m == 0xDD) {
            if (len != 2) return XMC_JPEG_E_MALFORMED;
            j->restart_interval = be16(s);
        } else if (m == 0xDA) {
            if (!j->have_sof) return XMC_JPEG_E_MALFORMED;
            if (scans >= XMC_JPEG_MAX_SCANS) return XMC_JPEG_E_SCANS;
            if (scans == 0) memset(coef, 0, (size_t)j->coef_count * sizeof(int16_t));    /* not before a scan is really there */
            bits_t b = {p, end, 0, 0, 0, 0};
            rc = decode_scan(j, s, len, &b, coef);
            p = b.p;
            ++scans;
        }
        /* APPn, COM, DNL, DHP, EXP, JPGn: skipped */
        if (rc) return rc;
    }
    if (!j->have_sof || scans == 0) return XMC_JPEG_E_MALFORMED;
    for (int c = 0; c < j->ncomp; ++c) {
        if (!j->comp[c].dc_seen) return XMC_JPEG_E_MALFORMED;           /* a component no scan coded */
        if (!j->qt_defined[j->comp[c].tq]) return XMC_JPEG_E_TABLE;
    }
    return 0;
}

static void fill_info(const jpeg_t* j, int32_t* info) {
    memset(info, 0, XMC_JPEG_INFO_WORDS * sizeof(int32_t));
    info[0] = j->width, info[1] = j->height, info[2] = j->ncomp, info[3] = j->process;
    info[4] = j->hmax, info[5] = j->vmax, info[6] = j->mcus_x, info[7] = j->mcus_y;
    info[8] = (int32_t)(j->coef_count * 2);         /* bytes of the coefficient buffer (<= 3 * 2 * (2^26 + padding)) */
    info[9] = j->ncomp * 64 * 2;                    /* bytes of the quantisation tables */
}

/* info: XMC_JPEG_INFO_WORDS int32 -- width, height, components, process (0 baseline, 1 extended, 2 progressive), luma
 * sampling h, v, MCUs per row, MCU rows, coefficient bytes, table bytes; the rest 0.  The planes follow each other in the
 * coefficient buffer: component c has (mcus_y * v_c) x (mcus_x * h_c) blocks of 64 int16. */
int xmc_jpeg_info(const void* data, int64_t n, int32_t* info) {
    jpeg_t j;
    if (!data || !info || n < 0) return XMC_JPEG_E_MALFORMED;
    int rc = decode(&j, (const uint8_t*)data, n, NULL, 0);
    if (rc) return rc;
    if (!j.have_sof) return XMC_JPEG_E_MALFORMED;
    fill_info(&j, info);
    return 0;
}

/* coef: coef_bytes >= info[8]; qt: qt_bytes >= info[9], uint16 [component][64] in natural order */
int xmc_jpeg_coefficients(const void* data, int64_t n, int16_t* coef, int64_t coef_bytes, uint16_t* qt, int64_t qt_bytes) {
    jpeg_t j;
    if (!data || !coef || !qt || n < 0 || coef_bytes < 0) return XMC_JPEG_E_MALFORMED;
    int rc = decode(&j, (const uint8_t*)data, n, coef, coef_bytes / 2);
    if (rc) return rc;
    if (qt_bytes < j.ncomp * 128) return XMC_JPEG_E_BUFFER;
    for (int c = 0; c < j.ncomp; ++c) memcpy(qt + 64 * c, j.qt[j.comp[c].tq], 128);
    return 0;
}
