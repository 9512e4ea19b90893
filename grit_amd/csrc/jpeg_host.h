// Host stage of the JPEG decoder (grit_jpeg_probe / grit_jpeg_entropy of include/grit_hip.h): marker parsing and the
// baseline Huffman decode.  Plain C++ without HIP, globals or allocation, so that jpeg.hip includes it and a stand-alone
// program can compile it on its own.  Every read of the input goes through an end pointer, every coefficient write through
// an index check; whatever the parser does not positively recognise is GRIT_ERR_UNSUPPORTED and the caller decodes with
// its host library.
//
// Accepted: SOF0, 8-bit, one interleaved scan, 8-bit quantisation tables, 1 component (decoded as 1x1) or 3 components taken for YCbCr
// by libjpeg's rule (JFIF marker; else Adobe transform 1; else component ids other than 'R','G','B') with luma 1x1, 2x1 or
// 2x2 over 1x1 chroma, DRI.  Coefficients leave de-zigzagged as int16, one plane of [block_rows][block_cols][64] per
// component, block counts padded to whole MCUs.
#ifndef GRIT_JPEG_HOST_H
#define GRIT_JPEG_HOST_H

#include <stdint.h>
#include <string.h>

#include "../../include/grit_hip.h"

namespace grit_jpeg {

static const uint8_t kNatural[64] = {  // zigzag position -> row-major position
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;
constexpr int kCoefBound = GRIT_JPEG_COEF_BOUND;

struct HuffSpec {  // a DHT table as it stands in the file
    uint8_t defined;
    uint8_t bits[17];
    uint8_t vals[256];
};

struct HuffTable {  // derived: lookahead of kLookBits bits, canonical ranges behind it
    uint16_t look[1 << kLookBits];  // (length << 8) | symbol; 0: the code is longer than kLookBits
    int32_t maxcode[18];            // largest code of each length, -1 if none; [17] ends every search
    int32_t valoff[17];             // index of the first symbol of that length minus its first code
    uint8_t vals[256];
};

struct Header {
    grit_jpeg_info info;
    HuffSpec dc[4], ac[4];
    uint8_t td[3], ta[3];
};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS.  GRIT_OK or GRIT_ERR_UNSUPPORTED.
static inline int parse_header(const uint8_t* data, long nbytes, Header* h) {
    memset(h, 0, sizeof(*h));
    if (nbytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return GRIT_ERR_UNSUPPORTED;
    uint8_t quant[4][64], quant_defined[4] = {0, 0, 0, 0};
    uint8_t comp_id[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    grit_jpeg_info& info = h->info;
    long pos = 2;
    for (;;) {
        if (pos + 2 > nbytes || data[pos] != 0xFF) return GRIT_ERR_UNSUPPORTED;
        while (pos + 1 < nbytes && data[pos + 1] == 0xFF) ++pos;  // fill bytes in front of a marker
        if (pos + 2 > nbytes) return GRIT_ERR_UNSUPPORTED;
        const int marker = data[pos + 1];
        pos += 2;
        if (marker == 0xD8 || marker == 0xD9 || marker == 0x01 || marker == 0x00 || (marker >= 0xD0 && marker <= 0xD7))
            return GRIT_ERR_UNSUPPORTED;  // nothing of these belongs in front of the scan
        if (pos + 2 > nbytes) return GRIT_ERR_UNSUPPORTED;
        const int len = be16(data + pos);
        if (len < 2 || pos + len > nbytes) return GRIT_ERR_UNSUPPORTED;
        const uint8_t* seg = data + pos + 2;
        const int n = len - 2;
        if (marker == 0xC0) {
            if (sof || n < 6) return GRIT_ERR_UNSUPPORTED;
            const int nc = seg[5];
            if (seg[0] != 8 || (nc != 1 && nc != 3) || n != 6 + 3 * nc) return GRIT_ERR_UNSUPPORTED;
            info.height = be16(seg + 1);
            info.width = be16(seg + 3);
            if (info.height <= 0 || info.width <= 0) return GRIT_ERR_UNSUPPORTED;  // height 0: DNL
            if ((long)info.height * info.width > GRIT_JPEG_MAX_PIXELS) return GRIT_ERR_UNSUPPORTED;  // the host library's own guard decides
            info.ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = seg[6 + 3 * c];
                info.hs[c] = seg[7 + 3 * c] >> 4;
                info.vs[c] = seg[7 + 3 * c] & 15;
                tq[c] = seg[8 + 3 * c];
                if (tq[c] > 3) return GRIT_ERR_UNSUPPORTED;
            }
            sof = true;
        } else if (marker >= 0xC1 && marker <= 0xCF && marker != 0xC4 && marker != 0xC8 && marker != 0xCC) {
            return GRIT_ERR_UNSUPPORTED;  // extended, progressive, lossless, arithmetic frames
        } else if (marker == 0xCC || marker == 0xDC || marker == 0xC8) {
            return GRIT_ERR_UNSUPPORTED;  // arithmetic conditioning, DNL, reserved
        } else if (marker == 0xC4) {
            int at = 0;
            while (at < n) {
                if (at + 17 > n) return GRIT_ERR_UNSUPPORTED;
                const int tc = seg[at] >> 4, th = seg[at] & 15;
                if (tc > 1 || th > 3) return GRIT_ERR_UNSUPPORTED;
                HuffSpec& t = tc ? h->ac[th] : h->dc[th];
                int count = 0;
                t.bits[0] = 0;
                for (int i = 1; i <= 16; ++i) count += (t.bits[i] = seg[at + i]);
                if (count > 256 || at + 17 + count > n) return GRIT_ERR_UNSUPPORTED;
                memset(t.vals, 0, sizeof(t.vals));
                memcpy(t.vals, seg + at + 17, count);
                t.defined = 1;
                at += 17 + count;
            }
        } else if (marker == 0xDB) {
            int at = 0;
            while (at < n) {
                if (at + 65 > n) return GRIT_ERR_UNSUPPORTED;  // also refuses 16-bit tables that end the segment
                const int pq = seg[at] >> 4, t = seg[at] & 15;
                if (pq != 0 || t > 3) return GRIT_ERR_UNSUPPORTED;
                memcpy(quant[t], seg + at + 1, 64);
                for (int k = 0; k < 64; ++k)
                    if (quant[t][k] == 0) return GRIT_ERR_UNSUPPORTED;  // keeps |coefficient| <= the bound, whatever the stream
                quant_defined[t] = 1;
                at += 65;
            }
        } else if (marker == 0xDD) {
            if (n != 2) return GRIT_ERR_UNSUPPORTED;
            info.restart_interval = be16(seg);
        } else if (marker == 0xE0) {
            if (n >= 14 && seg[0] == 'J' && seg[1] == 'F' && seg[2] == 'I' && seg[3] == 'F' && seg[4] == 0) jfif = true;
        } else if (marker == 0xEE) {
            if (n >= 12 && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') {
                adobe = true;
                adobe_transform = seg[11];
            }
        } else if (marker == 0xDA) {
            if (!sof || n < 1 || seg[0] != info.ncomp || n != 4 + 2 * info.ncomp) return GRIT_ERR_UNSUPPORTED;  // one interleaved scan
            for (int c = 0; c < info.ncomp; ++c) {
                if (seg[1 + 2 * c] != comp_id[c]) return GRIT_ERR_UNSUPPORTED;
                h->td[c] = seg[2 + 2 * c] >> 4;
                h->ta[c] = seg[2 + 2 * c] & 15;
                if (h->td[c] > 3 || h->ta[c] > 3 || !h->dc[h->td[c]].defined || !h->ac[h->ta[c]].defined || !quant_defined[tq[c]])
                    return GRIT_ERR_UNSUPPORTED;
            }
            const uint8_t* tail = seg + 1 + 2 * info.ncomp;
            if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return GRIT_ERR_UNSUPPORTED;
            pos += len;
            break;
        }  // every other segment (APPn, COM, unknown) is skipped
        pos += len;
    }
    grit_jpeg_info& i = h->info;
    if (i.ncomp == 1) {
        if (i.hs[0] < 1 || i.hs[0] > 4 || i.vs[0] < 1 || i.vs[0] > 4) return GRIT_ERR_UNSUPPORTED;
        i.hs[0] = i.vs[0] = 1;  // a scan of one component is not interleaved: one block per MCU whatever its factors say
    } else {
        if (i.hs[1] != 1 || i.vs[1] != 1 || i.hs[2] != 1 || i.vs[2] != 1) return GRIT_ERR_UNSUPPORTED;
        if (!((i.hs[0] == 1 && i.vs[0] == 1) || (i.hs[0] == 2 && i.vs[0] == 1) || (i.hs[0] == 2 && i.vs[0] == 2)))
            return GRIT_ERR_UNSUPPORTED;
        if (!jfif) {  // libjpeg's guess of the colour space
            if (adobe) {
                if (adobe_transform != 1) return GRIT_ERR_UNSUPPORTED;
            } else if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') {
                return GRIT_ERR_UNSUPPORTED;
            }
        }
    }
    i.hmax = i.hs[0];
    i.vmax = i.vs[0];
    i.mcu_cols = (i.width + 8 * i.hmax - 1) / (8 * i.hmax);
    i.mcu_rows = (i.height + 8 * i.vmax - 1) / (8 * i.vmax);
    long blocks = 0;
    for (int c = 0; c < i.ncomp; ++c) {
        i.block_cols[c] = i.mcu_cols * i.hs[c];
        i.block_rows[c] = i.mcu_rows * i.vs[c];
        blocks += (long)i.block_cols[c] * i.block_rows[c];
        for (int k = 0; k < 64; ++k) i.quant[64 * c + kNatural[k]] = quant[tq[c]][k];
    }
    i.coef_bytes = blocks * 128;
    i.plane_bytes = blocks * 64;
    i.scan_offset = pos;
    return GRIT_OK;
}

// jdhuff.c: jpeg_make_d_derived_tbl.  false: not a prefix code.
static inline bool derive(const HuffSpec& s, HuffTable* t) {
    uint8_t size[257];
    int n = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < s.bits[l]; ++i) {
            if (n >= 256) return false;
            size[n++] = (uint8_t)l;
        }
    memcpy(t->vals, s.vals, 256);
    memset(t->look, 0, sizeof(t->look));
    int32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (s.bits[l] == 0) {
            t->maxcode[l] = -1;
            t->valoff[l] = 0;
        } else {
            t->valoff[l] = p - code;
            for (int i = 0; i < s.bits[l]; ++i, ++p, ++code) {
                if (code >= (1 << l)) return false;
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l);
                    for (int f = 0; f < (1 << (kLookBits - l)); ++f) t->look[first + f] = (uint16_t)((l << 8) | s.vals[p]);
                }
            }
            t->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    t->maxcode[0] = -1;
    t->maxcode[17] = 0x7FFFFFFF;
    return true;
}

struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;  // the next `cnt` bits of the stream, from the top
    int cnt;
    int pad;  // how many of them, at the bottom, are zeros made up behind a marker or the end of the data
};

static inline void refill_slow(Bits& b);

// A symbol and the bits behind it take at most 16 + 15 of the buffer: refill below 32.  Afterwards cnt >= 57.
static inline void refill(Bits& b) {
    if (b.cnt >= 32) return;
    refill_slow(b);
}

static inline void refill_slow(Bits& b) {
    if (b.end - b.p >= 8 && b.pad == 0) {
        uint64_t v;
        memcpy(&v, b.p, 8);
        const uint64_t inv = ~v;
        if (((inv - 0x0101010101010101ULL) & ~inv & 0x8080808080808080ULL) == 0) {  // no 0xFF among the eight bytes
            v = __builtin_bswap64(v);
            const int nb = (64 - b.cnt) >> 3;
            b.buf |= (v >> b.cnt) & (~0ULL << (64 - b.cnt - 8 * nb));
            b.cnt += 8 * nb;
            b.p += nb;
            return;
        }
    }
    while (b.cnt <= 56) {
        uint64_t byte = 0;
        if (b.pad == 0 && b.p < b.end) {
            byte = *b.p;
            if (byte != 0xFF) {
                ++b.p;
            } else if (b.end - b.p >= 2 && b.p[1] == 0) {
                b.p += 2;
            } else {  // a marker (or a lone 0xFF at the end): the segment ends here
                byte = 0;
                b.pad += 8;
            }
        } else {
            b.pad += 8;
        }
        b.buf |= byte << (56 - b.cnt);
        b.cnt += 8;
    }
}

static inline void drop(Bits& b, int n) {
    b.buf <<= n;
    b.cnt -= n;
}

// One Huffman symbol; the caller has refilled.  -1: no such code.
static inline int symbol(Bits& b, const HuffTable& t) {
    const int e = t.look[b.buf >> (64 - kLookBits)];
    if (e) {
        drop(b, e >> 8);
        return e & 255;
    }
    int l = kLookBits + 1;
    int32_t code = (int32_t)(b.buf >> (64 - l));
    while (code > t.maxcode[l]) {
        ++l;
        code = (int32_t)(b.buf >> (64 - l));
    }
    if (l > 16) return -1;
    const int at = code + t.valoff[l];
    if (at < 0 || at > 255) return -1;
    drop(b, l);
    return t.vals[at];
}

static inline int extend(Bits& b, int s) {  // the s > 0 bits behind a symbol as a signed value
    const int v = (int)(b.buf >> (64 - s));
    drop(b, s);
    const int low = (v >> (s - 1)) - 1;  // all ones when the leading bit is 0: the negative half
    return v + (low & (1 - (1 << s)));
}

static inline int entropy(const uint8_t* data, long nbytes, const grit_jpeg_info* given, int16_t* coef, long coef_bytes) {
    Header h;
    int st = parse_header(data, nbytes, &h);
    if (st != GRIT_OK) return st;
    const grit_jpeg_info& info = h.info;
    if (given && memcmp(given, &info, sizeof(info)) != 0) return GRIT_ERR_BAD_ARG;  // not the probe of these bytes
    if (coef_bytes < info.coef_bytes) return GRIT_ERR_BAD_ARG;
    HuffTable dc[3], ac[3];
    for (int c = 0; c < info.ncomp; ++c)
        if (!derive(h.dc[h.td[c]], &dc[c]) || !derive(h.ac[h.ta[c]], &ac[c])) return GRIT_ERR_UNSUPPORTED;
    int16_t* plane[3] = {coef, coef, coef};
    for (int c = 1; c < info.ncomp; ++c) plane[c] = plane[c - 1] + (long)info.block_cols[c - 1] * info.block_rows[c - 1] * 64;
    const long total_elems = info.coef_bytes / 2;
    Bits b = {data + info.scan_offset, data + nbytes, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int until_restart = info.restart_interval, next_rst = 0;
    for (int my = 0; my < info.mcu_rows; ++my) {
        for (int mx = 0; mx < info.mcu_cols; ++mx) {
            if (info.restart_interval && until_restart == 0) {
                if (b.cnt < b.pad || b.cnt - b.pad >= 8) return GRIT_ERR_UNSUPPORTED;  // bits read past the end, or bytes left over
                if (b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD0 + next_rst) return GRIT_ERR_UNSUPPORTED;
                b.p += 2;
                b.buf = 0;
                b.cnt = b.pad = 0;
                next_rst = (next_rst + 1) & 7;
                until_restart = info.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            --until_restart;
            for (int c = 0; c < info.ncomp; ++c) {
                const int* q = info.quant + 64 * c;
                for (int by = 0; by < info.vs[c]; ++by) {
                    for (int bx = 0; bx < info.hs[c]; ++bx) {
                        const long at = (((long)my * info.vs[c] + by) * info.block_cols[c] + (long)mx * info.hs[c] + bx) * 64;
                        if (at < 0 || (plane[c] - coef) + at + 64 > total_elems) return GRIT_ERR_BAD_ARG;
                        int16_t* blk = plane[c] + at;
                        memset(blk, 0, 128);
                        refill(b);
                        int s = symbol(b, dc[c]);
                        if (s < 0 || s > 15) return GRIT_ERR_UNSUPPORTED;
                        if (s) pred[c] += extend(b, s);  // at most 16 + 15 of the 57 bits
                        if (pred[c] * q[0] > kCoefBound || pred[c] * q[0] < -kCoefBound) return GRIT_ERR_UNSUPPORTED;
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64; ++k) {
                            refill(b);
                            const int rs = symbol(b, ac[c]);
                            if (rs < 0) return GRIT_ERR_UNSUPPORTED;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;  // end of block
                                k += 15;
                                continue;
                            }
                            k += r;
                            if (k > 63) return GRIT_ERR_UNSUPPORTED;
                            const int v = extend(b, s);
                            const int pos = kNatural[k];
                            if (v * q[pos] > kCoefBound || v * q[pos] < -kCoefBound) return GRIT_ERR_UNSUPPORTED;
                            blk[pos] = (int16_t)v;
                        }
                        if (b.cnt < b.pad) return GRIT_ERR_UNSUPPORTED;  // the block read past the end of its segment
                    }
                }
            }
        }
    }
    // the scan must end where an EOI stands: no made-up bit consumed, less than a byte of padding left
    if (b.cnt < b.pad || b.cnt - b.pad >= 8) return GRIT_ERR_UNSUPPORTED;
    if (b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD9) return GRIT_ERR_UNSUPPORTED;
    return GRIT_OK;
}

}  // namespace grit_jpeg

#endif  // GRIT_JPEG_HOST_H
