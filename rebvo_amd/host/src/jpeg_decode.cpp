// jpeg_decode.cpp — the device JPEG decoder's three stages on the CPU: the marker parser (rebvo/jpeg_decode.h), the host instantiation of
// the chain walk (csrc/jpeg_entropy.h) and a plain restatement of the pixel stage over the functions the kernels call (csrc/jpeg_pixels.h).
// tests/test_jpeg_decode_cpu.py holds it to PIL's pixels; tools/make_jpeg_decode_golden.py counts a stream's populations with it.
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_pixels.h"

namespace {
using namespace rebvo::jpegdec;

struct HostSrc {
    const uint8_t *p;
    int byte(uint32_t pos) const { return p[pos]; }
};
struct HostSink {
    std::vector<int16_t> &coef;
    int16_t cur[64];
    long long *stats;   // [6] or null: codes longer than 8 bits, ZRL, blocks without EOB, largest DC category, largest AC category, blocks
    void begin_block() { memset(cur, 0, sizeof cur); }
    void put(int k, int v) { cur[k] = (int16_t)v; }
    void note(int what, int v) {
        if (!stats) return;
        if (what == kNoteCodeLength) stats[0] += v > 8;
        else if (what == kNoteZrl) stats[1]++;
        else if (what == kNoteNoEob) stats[2]++;
        else if (what == kNoteDcCategory) stats[3] = v > stats[3] ? v : stats[3];
        else if (what == kNoteAcCategory) stats[4] = v > stats[4] ? v : stats[4];
    }
    void end_block(int block) {
        memcpy(&coef[(size_t)block * 64], cur, sizeof cur);
        if (stats) stats[5]++;
    }
};
}  // namespace

// w > 0: the caller's frame size and cap (jpegdec::expect) are applied to the descriptor as edgehip_upload_jpeg applies them
extern "C" int rebvo_jpeg_probe_expect(const unsigned char *data, long long len, int w, int h, unsigned cap_bytes, void *info_out) {
    Stream s;
    parse(data, len < 0 ? 0 : (size_t)len, s);
    if (w > 0) expect(s, w, h, cap_bytes);
    if (info_out) { const Info i = info_of(s); memcpy(info_out, &i, sizeof i); }
    return s.reason;
}

extern "C" int rebvo_jpeg_probe(const unsigned char *data, long long len, void *info_out) {
    Stream s;
    parse(data, len < 0 ? 0 : (size_t)len, s);
    if (info_out) { const Info i = info_of(s); memcpy(info_out, &i, sizeof i); }
    return s.reason;
}

// -> the parser's reason code (nothing is decoded then), else 0 with *status = the walk's status (the largest over the stream's groups),
// w x h, and — when rgb has room — the pixels as the device writes them.  stats[6] (or null): see HostSink.  groups (or null): walks taken.
extern "C" int rebvo_jpeg_decode_staged(const unsigned char *data, long long len, unsigned char *rgb, long long cap, int *w, int *h, int *status,
                                        long long *stats, int *groups) {
    Stream s;
    if (parse(data, len < 0 ? 0 : (size_t)len, s)) return s.reason;
    if (w) *w = s.w;
    if (h) *h = s.h;
    const uint8_t *ecs = data + s.ecs_off;
    ChainPlan plan;
    plan_chains(ecs, s, plan);
    if (groups) *groups = plan.ngroups;
    std::vector<int16_t> coef((size_t)s.nblocks * 64, 0);
    HostSrc src = {ecs};
    HostSink sink = {coef, {0}, stats};
    if (stats) memset(stats, 0, 6 * sizeof *stats);
    const int nmcu = s.mcux * s.mcuy;
    int st = 0;
    for (int g = 0; g < plan.ngroups; g++) {
        const int first = g * plan.group_mcus, count = nmcu - first < plan.group_mcus ? nmcu - first : plan.group_mcus;
        const int e = chain_walk(s, first, count, plan.off[g], s.ecs_len, src, sink, nullptr);
        st = e > st ? e : st;
    }
    if (status) *status = st;
    if (!rgb || (long long)s.w * s.h * 3 > cap) return 0;
    std::vector<uint8_t> samples((size_t)s.nblocks * 64);
    for (int ci = 0; ci < s.ncomp; ci++) {
        const Comp &c = s.comp[ci];
        const uint16_t *q = s.q[c.tq];
        for (int b = 0; b < c.wblocks * c.hblocks; b++) {
            const int16_t *cf = &coef[(size_t)(c.block_base + b) * 64];
            int ws[64];
            for (int col = 0; col < 8; col++) {
                int in[8], o[8];
                for (int r = 0; r < 8; r++) in[r] = cf[8 * r + col] * (int)q[8 * r + col];
                px_idct_col(in, o);
                for (int r = 0; r < 8; r++) ws[8 * r + col] = o[r];
            }
            uint8_t *dst = &samples[(size_t)c.block_base * 64 + (size_t)(b / c.wblocks) * 8 * (c.wblocks * 8) + (size_t)(b % c.wblocks) * 8];
            for (int r = 0; r < 8; r++) px_idct_row(ws + 8 * r, dst + (size_t)r * c.wblocks * 8);
        }
    }
    for (int y = 0; y < s.h; y++)
        for (int x = 0; x < s.w; x++) {
            const uint32_t p = px_pixel(s, samples.data(), x, y);
            unsigned char *o = rgb + ((size_t)y * s.w + x) * 3;
            o[0] = p & 0xFF; o[1] = (p >> 8) & 0xFF; o[2] = p >> 16;
        }
    return 0;
}
