// Stand-alone sanitizer check of the JPEG host pass (dynamicvectorquantization_amd/csrc/jpeg_host.cpp): that file parses untrusted
// bytes, so it is built here with g++ alone under AddressSanitizer and UndefinedBehaviorSanitizer and fed whole files, every
// truncation of them, random corruptions and directed wrong-but-well-formed headers (over-subscribed, empty and 256-code Huffman
// tables, a 16-bit DQT, a scan naming undefined tables), each from a heap block of exactly the input's size (an over-read of one byte is
// caught) into a coefficient buffer of exactly the size dvq_jpeg_info reports.  CPU only; no GPU, no Python.
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import jpeg_math as jm, os; os.makedirs('/tmp/jpeg_cases', exist_ok=True); \
//              [open('/tmp/jpeg_cases/%s.jpg' % c[0], 'wb').write(jm.case_bytes(c[0])) for c in jm.CASES]"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp \
//       dynamicvectorquantization_amd/csrc/jpeg_host.cpp -o /tmp/jpeg_host_check
//   /tmp/jpeg_host_check /tmp/jpeg_cases/*.jpg
//
// Exit status 0 and a line per file when nothing was flagged; a sanitizer report aborts the run.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <utility>
#include <vector>

#include "../include/dvq_hip.h"

static char g_err[512];
void dvq_set_error(const char* fmt, ...) {      // misc.hip's in the library
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// one decode from exact-size heap blocks -> return code of the entropy pass (1: dvq_jpeg_info left the stream to another decoder)
static int run(const uint8_t* bytes, size_t n, int64_t capacity_delta, uint64_t* checksum) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    memcpy(data, bytes, n);
    dvq_jpeg_info_t info;
    int rc = dvq_jpeg_info(data, n, &info);
    if (rc != DVQ_OK) abort();
    int out = 1;
    // a corrupted frame header can name a 65535 x 65535 image: the caller owns the buffers, and this caller stops at 2^26 coefficients
    if (info.supported == DVQ_JPEG_SUPPORTED && info.coef_count <= ((int64_t)1 << 26)) {
        const int64_t cap = info.coef_count + capacity_delta;
        int16_t* coef = (int16_t*)malloc((size_t)(cap > 0 ? cap : 1) * sizeof(int16_t));
        uint16_t* qtab = (uint16_t*)malloc((size_t)info.components * 64 * sizeof(uint16_t));
        out = dvq_jpeg_entropy_decode(data, n, coef, cap, qtab);
        if (out == DVQ_OK && checksum) {
            uint64_t h = 1469598103934665603ull;
            for (int64_t i = 0; i < info.coef_count; ++i) h = (h ^ (uint16_t)coef[i]) * 1099511628211ull;
            *checksum = h;
        }
        free(coef);
        free(qtab);
    }
    free(data);
    return out;
}

// ---- directed cases: segments that are well formed as segments and wrong in what they say (random byte flips almost never make one:
// a raised count byte makes the segment's own length check fail first)
static const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// offset of the first SOS marker of a file that dvq_jpeg_info took (so the walk stays inside it)
static size_t find_sos(const std::vector<uint8_t>& b) {
    size_t pos = 2;
    for (;;) {
        while (b[pos] == 0xFF) ++pos;
        const int m = b[pos++];
        if (m == 0xDA) return pos - 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;
        pos += ((size_t)b[pos] << 8) | b[pos + 1];
    }
}

// the file with one more segment (marker, payload) in front of its SOS: a later table definition replaces an earlier one
static std::vector<uint8_t> with_segment(const std::vector<uint8_t>& b, int marker, const std::vector<uint8_t>& payload) {
    const size_t sos = find_sos(b), len = payload.size() + 2;
    std::vector<uint8_t> out(b.begin(), b.begin() + sos);
    out.push_back(0xFF);
    out.push_back((uint8_t)marker);
    out.push_back((uint8_t)(len >> 8));
    out.push_back((uint8_t)len);
    out.insert(out.end(), payload.begin(), payload.end());
    out.insert(out.end(), b.begin() + sos, b.end());
    return out;
}

// a DHT payload: class / id byte, counts[l] codes of length l (all other lengths empty), values 0, 1, 2, ... (mod 256)
static std::vector<uint8_t> dht(int tc_th, std::initializer_list<std::pair<int, int>> counts) {
    std::vector<uint8_t> p(17, 0);
    p[0] = (uint8_t)tc_th;
    int total = 0;
    for (auto& c : counts) {
        p[c.first] = (uint8_t)c.second;
        total += c.second;
    }
    for (int i = 0; i < total; ++i) p.push_back((uint8_t)i);
    return p;
}

static int directed(const char* name, const std::vector<uint8_t>& bytes, uint64_t whole_sum) {
    int bad = 0;
    auto expect = [&](const char* what, const std::vector<uint8_t>& file, int want, bool any = false) {
        uint64_t sum = 0;
        const int rc = run(file.data(), file.size(), 0, &sum);
        if (!any && rc != want) {
            fprintf(stderr, "%s: %s: return code %d, expected %d\n", name, what, rc, want);
            ++bad;
        }
        return sum;
    };
    // over-subscribed tables (more codes of a length than the length holds): DC and AC, at 1 bit, at the lookahead's edge, beyond it
    for (int tc_th : {0x00, 0x10}) {
        expect("6 codes of 1 bit", with_segment(bytes, 0xC4, dht(tc_th, {{1, 6}})), DVQ_EINVAL);
        expect("200 codes of 1 bit", with_segment(bytes, 0xC4, dht(tc_th, {{1, 200}})), DVQ_EINVAL);
        expect("3 codes of 1 bit", with_segment(bytes, 0xC4, dht(tc_th, {{1, 3}})), DVQ_EINVAL);
        expect("full at 1 bit + 5 codes of 9 bits", with_segment(bytes, 0xC4, dht(tc_th, {{1, 2}, {9, 5}})), DVQ_EINVAL);
        expect("full at 1 bit + 1 code of 10 bits", with_segment(bytes, 0xC4, dht(tc_th, {{1, 2}, {10, 1}})), DVQ_EINVAL);
        expect("full at 1 bit + 1 code of 16 bits", with_segment(bytes, 0xC4, dht(tc_th, {{1, 2}, {16, 1}})), DVQ_EINVAL);
        expect("1 code of 1 bit + 255 codes of 8 bits", with_segment(bytes, 0xC4, dht(tc_th, {{1, 1}, {8, 255}})), DVQ_EINVAL);
        expect("an empty table", with_segment(bytes, 0xC4, dht(tc_th, {})), DVQ_EINVAL);
    }
    // exactly 256 codes, a complete code of 8 bits: a DC table with symbols above 15 is refused, an AC table is legal to build
    expect("DC table of 256 codes", with_segment(bytes, 0xC4, dht(0x00, {{8, 255}, {9, 1}})), DVQ_EINVAL);
    expect("AC table of 256 codes", with_segment(bytes, 0xC4, dht(0x10, {{8, 255}, {9, 1}})), 0, true);
    // the luma quantisation table again with 16-bit entries: the same coefficients come out
    {
        std::vector<uint8_t> copy(bytes);
        dvq_jpeg_info_t info;
        dvq_jpeg_info(copy.data(), copy.size(), &info);
        std::vector<int16_t> coef((size_t)info.coef_count);
        std::vector<uint16_t> q((size_t)info.components * 64);
        dvq_jpeg_entropy_decode(copy.data(), copy.size(), coef.data(), info.coef_count, q.data());
        std::vector<uint8_t> p(1, (uint8_t)(0x10 | info.qtab_index[0]));
        for (int k = 0; k < 64; ++k) {
            p.push_back((uint8_t)(q[NATURAL[k]] >> 8));
            p.push_back((uint8_t)q[NATURAL[k]]);
        }
        if (expect("16-bit DQT", with_segment(bytes, 0xDB, p), DVQ_OK) != whole_sum) {
            fprintf(stderr, "%s: a 16-bit DQT with the same values changed the coefficients\n", name);
            ++bad;
        }
    }
    // a scan that names Huffman tables nobody defined: dvq_jpeg_info leaves the stream alone
    {
        std::vector<uint8_t> f(bytes);
        f[find_sos(f) + 6] = 0x33;      // marker 2, length 2, component count 1, component id 1 -> its table byte
        expect("SOS with undefined tables", f, 1);
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> bytes;
        uint8_t buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
        fclose(f);
        uint64_t sum = 0;
        const int whole = run(bytes.data(), bytes.size(), 0, &sum);
        if (whole != DVQ_OK) {
            fprintf(stderr, "%s: whole file not decoded (%d): %s\n", argv[a], whole, g_err);
            return 1;
        }
        if (run(bytes.data(), bytes.size(), -1, nullptr) != DVQ_EWORKSPACE) {
            fprintf(stderr, "%s: a coefficient buffer one element short was not refused\n", argv[a]);
            return 1;
        }
        if (directed(argv[a], bytes, sum)) return 1;
        // every truncation (large files: every offset of the first and last 4 KiB, every 97th in between)
        size_t cuts = 0, cut_ok = 0;
        for (size_t n = 0; n < bytes.size(); n += (n < 4096 || n + 4096 >= bytes.size()) ? 1 : 97) {
            cut_ok += run(bytes.data(), n, 0, nullptr) == DVQ_OK;
            ++cuts;
        }
        // random corruption: 1 .. 4 bytes anywhere in the file, headers and tables included
        size_t flips = 0, flip_ok = 0;
        uint32_t s = 12345u + (uint32_t)a;
        std::vector<uint8_t> bad;
        for (int it = 0; it < 3000; ++it) {
            bad = bytes;
            const int k = 1 + (int)((s = s * 1664525u + 1013904223u) >> 30);
            for (int j = 0; j < k; ++j) {
                const uint32_t pos = (s = s * 1664525u + 1013904223u) % (uint32_t)bad.size();
                bad[pos] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
            }
            flip_ok += run(bad.data(), bad.size(), 0, nullptr) == DVQ_OK;
            ++flips;
        }
        printf("%s: %zu bytes, coefficients fnv %016llx; %zu truncations (%zu decoded), %zu corruptions (%zu decoded)\n", argv[a],
               bytes.size(), (unsigned long long)sum, cuts, cut_ok, flips, flip_ok);
    }
    printf("jpeg_host_check: clean\n");
    return 0;
}
