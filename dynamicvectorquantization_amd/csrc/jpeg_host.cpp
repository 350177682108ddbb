// Host pass of the device JPEG decode (docs/design/23-device-jpeg.md): marker parsing and the Huffman pass of a baseline /
// extended-sequential JPEG -- the one serial part of a decode.  Everything after the coefficients (dequantisation, inverse DCT,
// chroma upsampling, colour conversion) runs in csrc/jpeg.hip.
//
// Plain C++ with no HIP dependence: the file also compiles with g++ alone (tools/jpeg_host_check.cpp builds it under
// AddressSanitizer).  It parses untrusted bytes: every read is checked against [data, data + n), every write against the caller's
// capacity; nothing is allocated and nothing is kept between calls.
#include <stdint.h>
#include <string.h>

#include "../../include/dvq_hip.h"

void dvq_set_error(const char* fmt, ...);     // misc.hip; a stand-alone build supplies its own

namespace {

// zigzag index -> natural (row-major) position
const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec {
    bool defined;
    uint8_t bits[17];      // bits[l]: number of codes of length l
    uint8_t vals[256];
    int nvals;
};

struct Frame {
    int w, h, nc, ri;
    int cid[4], hs[4], vs[4], tq[4], td[4], ta[4];
    bool qdef[4];
    uint16_t q[4][64];     // natural order
    HuffSpec dc[4], ac[4];
    size_t scan_off;       // first byte of the entropy-coded segment
    bool sof_seen, jfif, adobe;
    int adobe_transform;
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// -> DVQ_JPEG_* reason (0: a stream this decoder takes).  Fills what it has seen so far either way.
int parse_header(const uint8_t* data, size_t n, Frame& f) {
    memset(&f, 0, sizeof(f));
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return DVQ_JPEG_NOT_JPEG;
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n || data[pos] != 0xFF) return DVQ_JPEG_MALFORMED;
        while (pos < n && data[pos] == 0xFF) ++pos;                   // fill bytes
        if (pos >= n) return DVQ_JPEG_MALFORMED;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;          // no payload
        if (m == 0x00 || m == 0xD9) return DVQ_JPEG_MALFORMED;        // EOI before any scan
        if (pos + 2 > n) return DVQ_JPEG_MALFORMED;
        const size_t len = (size_t)be16(data + pos);
        if (len < 2 || pos + len > n) return DVQ_JPEG_MALFORMED;
        const uint8_t* seg = data + pos + 2;
        const size_t slen = len - 2;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {          // SOFn
            if (f.sof_seen || slen < 6) return DVQ_JPEG_MALFORMED;
            const int prec = seg[0], nc = seg[5];
            f.h = be16(seg + 1);
            f.w = be16(seg + 3);
            f.nc = nc;
            if (slen != 6 + 3 * (size_t)nc) return DVQ_JPEG_MALFORMED;
            for (int i = 0; i < nc && i < 4; ++i) {
                f.cid[i] = seg[6 + 3 * i];
                f.hs[i] = seg[7 + 3 * i] >> 4;
                f.vs[i] = seg[7 + 3 * i] & 15;
                f.tq[i] = seg[8 + 3 * i];
            }
            if (m == 0xC2) return DVQ_JPEG_PROGRESSIVE;
            if (m >= 0xC9) return DVQ_JPEG_ARITHMETIC;
            if (m != 0xC0 && m != 0xC1) return DVQ_JPEG_SOF_KIND;     // lossless, hierarchical
            if (prec != 8) return DVQ_JPEG_PRECISION;
            if (f.w == 0 || f.h == 0) return DVQ_JPEG_MALFORMED;      // height 0: defined later by a DNL marker
            if (nc != 1 && nc != 3) return DVQ_JPEG_COMPONENTS;
            for (int i = 0; i < nc; ++i)
                if (f.hs[i] < 1 || f.hs[i] > 4 || f.vs[i] < 1 || f.vs[i] > 4 || f.tq[i] > 3) return DVQ_JPEG_MALFORMED;
            f.sof_seen = true;
        } else if (m == 0xDB) {                                       // DQT
            size_t o = 0;
            while (o < slen) {
                const int pq = seg[o] >> 4, tq = seg[o] & 15;
                ++o;
                if (pq > 1 || tq > 3 || o + (size_t)64 * (pq + 1) > slen) return DVQ_JPEG_MALFORMED;
                for (int k = 0; k < 64; ++k) {
                    f.q[tq][NATURAL[k]] = (uint16_t)(pq ? be16(seg + o + 2 * k) : seg[o + k]);
                }
                o += (size_t)64 * (pq + 1);
                f.qdef[tq] = true;
            }
        } else if (m == 0xC4) {                                       // DHT
            size_t o = 0;
            while (o < slen) {
                if (o + 17 > slen) return DVQ_JPEG_MALFORMED;
                const int tc = seg[o] >> 4, th = seg[o] & 15;
                if (tc > 1 || th > 3) return DVQ_JPEG_MALFORMED;
                HuffSpec& s = tc ? f.ac[th] : f.dc[th];
                int total = 0;
                s.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (s.bits[l] = seg[o + l]);
                o += 17;
                if (total > 256 || o + (size_t)total > slen) return DVQ_JPEG_MALFORMED;
                memcpy(s.vals, seg + o, (size_t)total);
                s.nvals = total;
                s.defined = true;
                o += (size_t)total;
            }
        } else if (m == 0xDD) {                                       // DRI
            if (slen < 2) return DVQ_JPEG_MALFORMED;
            f.ri = be16(seg);
        } else if (m == 0xE0) {
            if (slen >= 5 && memcmp(seg, "JFIF", 5) == 0) f.jfif = true;
        } else if (m == 0xEE) {
            if (slen >= 12 && memcmp(seg, "Adobe", 5) == 0) {
                f.adobe = true;
                f.adobe_transform = seg[11];
            }
        } else if (m == 0xDA) {                                       // SOS
            if (!f.sof_seen || slen < 1) return DVQ_JPEG_MALFORMED;
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || slen != 1 + 2 * (size_t)ns + 3) return DVQ_JPEG_MALFORMED;
            if (ns != f.nc) return DVQ_JPEG_MULTISCAN;
            for (int i = 0; i < ns; ++i) {
                if (seg[1 + 2 * i] != f.cid[i]) return DVQ_JPEG_MALFORMED;
                f.td[i] = seg[2 + 2 * i] >> 4;
                f.ta[i] = seg[2 + 2 * i] & 15;
                if (f.td[i] > 3 || f.ta[i] > 3 || !f.dc[f.td[i]].defined || !f.ac[f.ta[i]].defined || !f.qdef[f.tq[i]])
                    return DVQ_JPEG_MALFORMED;
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return DVQ_JPEG_MALFORMED;
            if (f.nc == 3) {
                if (f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return DVQ_JPEG_SAMPLING;
                const int hv = f.hs[0] * 16 + f.vs[0];
                if (hv != 0x11 && hv != 0x21 && hv != 0x22) return DVQ_JPEG_SAMPLING;
                // colour space by libjpeg's rules: an Adobe marker names the transform; JFIF means YCbCr; without either, the
                // component ids 'R' 'G' 'B' mean RGB
                if (f.adobe ? f.adobe_transform != 1 : (!f.jfif && f.cid[0] == 'R' && f.cid[1] == 'G' && f.cid[2] == 'B'))
                    return DVQ_JPEG_COLORSPACE;
            } else {
                f.hs[0] = f.vs[0] = 1;      // a one-component scan is not interleaved: its sampling factors mean nothing
            }
            f.scan_off = pos + len;
            return DVQ_JPEG_SUPPORTED;
        }
        pos += len;
    }
}

inline int mcus_x(const Frame& f) { return (f.w + 8 * f.hs[0] - 1) / (8 * f.hs[0]); }
inline int mcus_y(const Frame& f) { return (f.h + 8 * f.vs[0] - 1) / (8 * f.vs[0]); }
inline int64_t coef_count(const Frame& f) {
    int64_t blocks = 0;
    for (int c = 0; c < f.nc; ++c) blocks += (int64_t)mcus_x(f) * f.hs[c] * mcus_y(f) * f.vs[c];
    return blocks * 64;
}

// ---- Huffman tables: LOOK bits of lookahead resolve every code of up to LOOK bits in one table read; longer codes walk maxcode[]
constexpr int LOOK = 9;

struct HuffTab {
    uint16_t look[1 << LOOK];      // (length << 8) | symbol for a code of <= LOOK bits that starts the index; 0: longer code
    int16_t fast_ac[1 << LOOK];    // AC only: value * 256 + run * 16 + (code length + magnitude bits) when both fit in LOOK bits; 0: none
    int32_t maxcode[18];           // largest code of each length, -1 where there is none; [17]: sentinel
    int32_t delta[17];             // index into vals = code + delta[length]
    uint8_t vals[256];
    int nvals;
};

bool build_table(const HuffSpec& s, bool is_dc, HuffTab& t) {
    memset(&t, 0, sizeof(t));
    memcpy(t.vals, s.vals, sizeof(t.vals));
    t.nvals = s.nvals;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.delta[l] = k - code;
        for (int i = 0; i < s.bits[l]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;      // more codes than the length holds: refused BEFORE the code indexes look[]
            if (l <= LOOK) {
                const int first = code << (LOOK - l);
                for (int j = 0; j < (1 << (LOOK - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | s.vals[k]);
            }
        }
        t.maxcode[l] = s.bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    if (is_dc) {
        for (int i = 0; i < s.nvals; ++i)
            if (s.vals[i] > 15) return false;
        return true;
    }
    for (int i = 0; i < (1 << LOOK); ++i) {
        const int e = t.look[i];
        if (!e) continue;
        const int len = e >> 8, run = (e >> 4) & 15, mag = e & 15;
        if (mag && len + mag <= LOOK) {
            int v = ((i << len) & ((1 << LOOK) - 1)) >> (LOOK - mag);
            if (v < (1 << (mag - 1))) v -= (1 << mag) - 1;
            if (v >= -128 && v <= 127) t.fast_ac[i] = (int16_t)(v * 256 + run * 16 + len + mag);
        }
    }
    return true;
}

// ---- bit reader over the byte-stuffed entropy segment: a 64-bit accumulator, most significant bit first.  It never passes a
// marker: from there on (and past the end of the data) it feeds zero bits and counts them, and the caller checks at the end of
// every restart interval that none of them was consumed
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int bits;          // valid bits at the top of acc; the bits below them are zero
    int64_t fake;      // how many of them are made-up zeros (always the last ones)
};

__attribute__((always_inline)) inline void refill(Bits& b) {
    if (b.end - b.p >= 8) {
        uint64_t v;
        memcpy(&v, b.p, 8);
        v = __builtin_bswap64(v);
        const uint64_t t = ~v;                                                         // a zero byte of t is an 0xFF byte of v
        if (!((t - 0x0101010101010101ull) & ~t & 0x8080808080808080ull)) {
            const int nb = (64 - b.bits) >> 3, keep = b.bits + 8 * nb;               // whole bytes only
            b.acc = (b.acc | (v >> b.bits)) & (~0ull << (64 - keep));
            b.p += nb;
            b.bits = keep;
            return;
        }
    }
    while (b.bits <= 56) {
        if (b.p >= b.end) break;
        const unsigned byte = *b.p;
        if (byte == 0xFF) {
            if (b.end - b.p >= 2 && b.p[1] == 0) b.p += 2;      // stuffed zero
            else break;                                          // a marker (or a lone 0xFF at the end)
        } else {
            ++b.p;
        }
        b.acc |= (uint64_t)byte << (56 - b.bits);
        b.bits += 8;
    }
    if (b.bits <= 56) {
        b.fake += 64 - b.bits;
        b.bits = 64;
    }
}

#define DVQ_JPEG_NEED(b)               \
    do {                               \
        if ((b).bits < 32) refill(b);  \
    } while (0)

__attribute__((always_inline)) inline unsigned peek(const Bits& b, int n) { return (unsigned)(b.acc >> (64 - n)); }
__attribute__((always_inline)) inline void skip(Bits& b, int n) {
    b.acc <<= n;
    b.bits -= n;
}
// n in 1..16 magnitude bits -> signed value (ITU T.81 F.2.2.1 EXTEND)
__attribute__((always_inline)) inline int receive_extend(Bits& b, int n) {
    const int v = (int)peek(b, n);
    skip(b, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// -> symbol, or -1 for a bit pattern that is no code of the table.  At least 16 valid bits are in the accumulator
__attribute__((always_inline)) inline int decode_symbol(Bits& b, const HuffTab& t) {
    const int e = t.look[peek(b, LOOK)];
    if (e) {
        skip(b, e >> 8);
        return e & 255;
    }
    const int c16 = (int)peek(b, 16);
    for (int l = LOOK + 1; l <= 16; ++l) {
        const int c = c16 >> (16 - l);
        if (c <= t.maxcode[l]) {
            const int idx = c + t.delta[l];
            if (idx < 0 || idx >= t.nvals) return -1;
            skip(b, l);
            return t.vals[idx];
        }
    }
    return -1;
}

// one 8x8 block into `blk` (zeroed by the caller), natural order
__attribute__((always_inline)) inline bool decode_block(Bits& b, const HuffTab& dc, const HuffTab& ac, int& pred, int16_t* blk) {
    DVQ_JPEG_NEED(b);
    const int s = decode_symbol(b, dc);
    if (s < 0) return false;
    if (s) {
        DVQ_JPEG_NEED(b);
        pred = (int16_t)(pred + receive_extend(b, s));
    }
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        DVQ_JPEG_NEED(b);
        const int fa = ac.fast_ac[peek(b, LOOK)];
        if (fa) {
            k += (fa >> 4) & 15;
            if (k > 63) return false;
            skip(b, fa & 15);
            blk[NATURAL[k++]] = (int16_t)(fa >> 8);
            continue;
        }
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return false;
        const int r = rs >> 4, m = rs & 15;
        if (m == 0) {
            if (r != 15) break;      // end of block
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return false;
        blk[NATURAL[k++]] = (int16_t)receive_extend(b, m);      // code <= 16 bits + m <= 15 bits: within the 32 the check above left
    }
    return true;
}

}  // namespace

extern "C" {

int dvq_jpeg_info(const uint8_t* data, size_t n, dvq_jpeg_info_t* info) {
    if (!data || !info) {
        dvq_set_error("dvq_jpeg_info: null pointer");
        return DVQ_EINVAL;
    }
    Frame f;
    const int reason = parse_header(data, n, f);
    memset(info, 0, sizeof(*info));
    info->width = f.w;
    info->height = f.h;
    info->components = f.nc;
    info->restart_interval = f.ri;
    for (int c = 0; c < 4 && c < f.nc; ++c) {
        info->h_samp[c] = f.hs[c];
        info->v_samp[c] = f.vs[c];
        info->qtab_index[c] = f.tq[c];
    }
    info->supported = reason;
    info->coef_count = reason == DVQ_JPEG_SUPPORTED ? coef_count(f) : 0;
    return DVQ_OK;
}

int dvq_jpeg_entropy_decode(const uint8_t* data, size_t n, int16_t* coef, int64_t coef_capacity, uint16_t* qtab) {
    if (!data || !coef || !qtab) {
        dvq_set_error("dvq_jpeg_entropy_decode: null pointer");
        return DVQ_EINVAL;
    }
    Frame f;
    const int reason = parse_header(data, n, f);
    if (reason != DVQ_JPEG_SUPPORTED) {
        dvq_set_error("dvq_jpeg_entropy_decode: not a supported JPEG stream (reason %d of dvq_jpeg_info)", reason);
        return DVQ_EINVAL;
    }
    const int64_t count = coef_count(f);
    if (coef_capacity < count) {
        dvq_set_error("dvq_jpeg_entropy_decode: coef_capacity %lld < %lld coefficients", (long long)coef_capacity, (long long)count);
        return DVQ_EWORKSPACE;
    }
    HuffTab dc[4], ac[4];      // built for the tables the scan names only
    bool have_dc[4] = {false, false, false, false}, have_ac[4] = {false, false, false, false};
    for (int c = 0; c < f.nc; ++c) {
        if (!have_dc[f.td[c]] && !build_table(f.dc[f.td[c]], true, dc[f.td[c]])) {
            dvq_set_error("dvq_jpeg_entropy_decode: invalid DC Huffman table %d", f.td[c]);
            return DVQ_EINVAL;
        }
        have_dc[f.td[c]] = true;
        if (!have_ac[f.ta[c]] && !build_table(f.ac[f.ta[c]], false, ac[f.ta[c]])) {
            dvq_set_error("dvq_jpeg_entropy_decode: invalid AC Huffman table %d", f.ta[c]);
            return DVQ_EINVAL;
        }
        have_ac[f.ta[c]] = true;
    }
    for (int c = 0; c < f.nc; ++c) memcpy(qtab + 64 * c, f.q[f.tq[c]], 64 * sizeof(uint16_t));
    memset(coef, 0, (size_t)count * sizeof(int16_t));

    const int mx = mcus_x(f), my = mcus_y(f);
    int16_t* base[4];
    int bcols[4];
    {
        int64_t off = 0;
        for (int c = 0; c < f.nc; ++c) {
            base[c] = coef + off;
            bcols[c] = mx * f.hs[c];
            off += (int64_t)bcols[c] * my * f.vs[c] * 64;
        }
    }
    Bits b = {data + f.scan_off, data + n, 0, 0, 0};
    int pred[4] = {0, 0, 0, 0};
    int64_t mcu = 0;
    int rst = 0;
    for (int y = 0; y < my; ++y) {
        for (int x = 0; x < mx; ++x, ++mcu) {
            if (f.ri && mcu && mcu % f.ri == 0) {
                if (b.fake > b.bits) {
                    dvq_set_error("dvq_jpeg_entropy_decode: entropy data ends before MCU %lld", (long long)mcu);
                    return DVQ_EINVAL;
                }
                // whatever is left of the interval is padding; the next marker must be the restart marker in sequence
                const uint8_t* p = b.p;
                while (b.end - p >= 2 && !(p[0] == 0xFF && p[1] != 0 && p[1] != 0xFF)) ++p;
                if (b.end - p < 2 || p[1] != 0xD0 + (rst & 7)) {
                    dvq_set_error("dvq_jpeg_entropy_decode: restart marker %d missing before MCU %lld", rst & 7, (long long)mcu);
                    return DVQ_EINVAL;
                }
                ++rst;
                b.p = p + 2;
                b.acc = 0;
                b.bits = 0;
                b.fake = 0;
                pred[0] = pred[1] = pred[2] = pred[3] = 0;
            }
            for (int c = 0; c < f.nc; ++c) {
                const HuffTab& tdc = dc[f.td[c]];
                const HuffTab& tac = ac[f.ta[c]];
                for (int v = 0; v < f.vs[c]; ++v) {
                    for (int h = 0; h < f.hs[c]; ++h) {
                        int16_t* blk = base[c] + ((int64_t)(y * f.vs[c] + v) * bcols[c] + (x * f.hs[c] + h)) * 64;
                        if (!decode_block(b, tdc, tac, pred[c], blk)) {
                            dvq_set_error("dvq_jpeg_entropy_decode: corrupt entropy data in MCU %lld", (long long)mcu);
                            return DVQ_EINVAL;
                        }
                    }
                }
            }
        }
    }
    if (b.fake > b.bits) {
        dvq_set_error("dvq_jpeg_entropy_decode: entropy data ends before the last MCU is complete");
        return DVQ_EINVAL;
    }
    return DVQ_OK;
}

}  // extern "C"
