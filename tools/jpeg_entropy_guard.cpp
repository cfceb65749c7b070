// jpeg_entropy_guard.cpp — the chain walk of the device JPEG decoder (rebvo_amd/csrc/jpeg_entropy.h) on the CPU, held to its bounds.
// A stand-alone program: tests/test_jpeg_decode_cpu.py builds it with the host compiler, together with the host reader
// (rebvo_amd/host/src/jpeg_reader.cpp), and gives it the fixtures' streams as files:
//     jpeg_entropy_guard file.jpg ... [--corrupt file.jpg ...]
// Every run of the walk works on exact-size heap copies — the entropy-coded segment, the descriptor (the tables) and the coefficient
// region each in an allocation of its own with canary bands on both sides — through a source that refuses a position outside the
// segment and a sink that refuses a block outside the region.  It runs on every file as it is and on a few thousand seeded corruptions
// of them: byte flips, truncation at every eighth byte, an early EOI.  Checked on every run: canaries intact; no refused access; exactly
// one end_block per block of the stream and at most 64 puts per block (the iteration bound); a nonzero status wherever the host reader
// reports an error; status 0 and the coefficients of the uncorrupted run wherever the corruption lies behind the last byte that run
// consumed.  The files behind --corrupt are walked as they are and must end in bounds with a nonzero status: the two corrupt streams the
// device test of the status reports uses (tests/jpeg_decode_fixtures.py) pass through here first.
// Prints one summary line; exit status 0 when every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "jpeg_entropy.h"

extern "C" int rebvo_decode_jpeg(const unsigned char *data, long long len, unsigned char *rgb, long long cap, int *w, int *h);

using namespace rebvo::jpegdec;

namespace {
constexpr size_t kBand = 64;
constexpr uint8_t kCanary = 0xA5;

struct Banded {   // `size` bytes between two canary bands, in one exact-size allocation
    uint8_t *raw = nullptr;
    size_t size = 0;
    explicit Banded(size_t n) : raw((uint8_t *)malloc(n + 2 * kBand)), size(n) { memset(raw, kCanary, n + 2 * kBand); }
    ~Banded() { free(raw); }
    Banded(const Banded &) = delete;
    uint8_t *data() { return raw + kBand; }
    bool intact() const {
        for (size_t i = 0; i < kBand; i++)
            if (raw[i] != kCanary || raw[kBand + size + i] != kCanary) return false;
        return true;
    }
};

struct Violations { long reads = 0, blocks = 0, puts = 0; };

struct GuardSrc {
    const uint8_t *p;
    uint32_t len;
    Violations *v;
    int byte(uint32_t pos) {
        if (pos >= len) { v->reads++; return 0; }
        return p[pos];
    }
};
struct GuardSink {
    int16_t *coef;
    int nblocks;
    Violations *v;
    std::vector<uint8_t> seen;
    int16_t cur[64];
    int puts = 0;
    long ended = 0;
    void begin_block() { memset(cur, 0, sizeof cur); puts = 0; }
    void put(int k, int val) {
        if (k < 0 || k > 63 || ++puts > 64) { v->puts++; return; }
        cur[k] = (int16_t)val;
    }
    void note(int, int) {}
    void end_block(int block) {
        ended++;
        if (block < 0 || block >= nblocks || seen[block]) { v->blocks++; return; }
        seen[block] = 1;
        memcpy(coef + (size_t)block * 64, cur, sizeof cur);
    }
};

struct Run {
    int reason = 0, status = 0;
    uint32_t ecs_off = 0, ecs_len = 0, end_pos = 0;   // end_pos: the furthest byte of the segment any group consumed
    int w = 0, h = 0, nblocks = 0, groups = 0;
    std::vector<int16_t> coef;
    bool ok = true;   // every bound held
};

Run run_walk(const std::vector<uint8_t> &file) {
    Run r;
    Banded in(file.size());
    memcpy(in.data(), file.data(), file.size());
    Banded tab(sizeof(Stream));
    Stream &s = *new (tab.data()) Stream;
    r.reason = parse(in.data(), file.size(), s);
    if (r.reason) { r.ok = in.intact() && tab.intact(); return r; }
    r.ecs_off = s.ecs_off; r.ecs_len = s.ecs_len; r.w = s.w; r.h = s.h; r.nblocks = s.nblocks;
    if ((size_t)s.ecs_off + s.ecs_len > file.size() || s.nblocks < 1 || s.nblocks > 3 * 2048 * 2048) { r.ok = false; return r; }
    Banded ecs(s.ecs_len);   // the segment alone, exact size: a read past it leaves the allocation
    memcpy(ecs.data(), in.data() + s.ecs_off, s.ecs_len);
    Banded coef((size_t)s.nblocks * 128);
    memset(coef.data(), 0, coef.size);
    ChainPlan plan;
    plan_chains(ecs.data(), s, plan);
    r.groups = plan.ngroups;
    Violations v;
    GuardSrc src = {ecs.data(), s.ecs_len, &v};
    GuardSink sink = {(int16_t *)coef.data(), s.nblocks, &v, std::vector<uint8_t>((size_t)s.nblocks, 0), {0}};
    const int nmcu = s.mcux * s.mcuy;
    if (plan.ngroups < 1 || plan.ngroups > kMaxGroups || (long long)plan.ngroups * plan.group_mcus < nmcu) r.ok = false;
    for (int g = 0; g < plan.ngroups && r.ok; g++) {
        const int first = g * plan.group_mcus, count = nmcu - first < plan.group_mcus ? nmcu - first : plan.group_mcus;
        if (plan.off[g] > s.ecs_len) { r.ok = false; break; }
        uint32_t end = 0;
        const int st = chain_walk(s, first, count, plan.off[g], s.ecs_len, src, sink, &end);
        if (st < 0 || st > 4 || end > s.ecs_len) r.ok = false;
        r.status = st > r.status ? st : r.status;
        r.end_pos = end > r.end_pos ? end : r.end_pos;
    }
    if (v.reads || v.blocks || v.puts || sink.ended != s.nblocks) r.ok = false;   // one end_block per block: the outer bound, met exactly
    if (!in.intact() || !tab.intact() || !ecs.intact() || !coef.intact()) r.ok = false;
    r.coef.assign((int16_t *)coef.data(), (int16_t *)coef.data() + (size_t)s.nblocks * 64);
    return r;
}

bool host_reader_fails(const std::vector<uint8_t> &file) { return rebvo_decode_jpeg(file.data(), (long long)file.size(), nullptr, 0, nullptr, nullptr) != 0; }

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

struct Totals { long runs = 0, refused = 0, nonzero = 0, host_errors = 0, behind = 0, failures = 0; };

// one corrupted variant against the uncorrupted run `base`; `at`: the first byte that differs from the original
bool check_variant(const char *what, const std::string &name, const std::vector<uint8_t> &file, size_t at, const Run &base, Totals &t) {
    const Run r = run_walk(file);
    t.runs++;
    bool ok = r.ok;
    if (r.reason) { t.refused++; }
    else {
        t.nonzero += r.status != 0;
        if (host_reader_fails(file)) {
            t.host_errors++;
            if (r.status == 0) ok = false;
        }
        const bool same_header = r.ecs_off == base.ecs_off && r.w == base.w && r.h == base.h && r.nblocks == base.nblocks && at >= base.ecs_off;
        if (same_header && at >= (size_t)base.ecs_off + base.end_pos && (base.groups == 1 || at >= (size_t)base.ecs_off + base.ecs_len)) {
            t.behind++;
            if (r.status != 0 || r.coef != base.coef) ok = false;
        }
    }
    if (!ok) {
        t.failures++;
        fprintf(stderr, "FAILED %s of %s at byte %zu: reason %d status %d bounds %d\n", what, name.c_str(), at, r.reason, r.status, (int)r.ok);
    }
    return ok;
}

}  // namespace

int main(int argc, char **argv) {
    bool corrupt = false;
    Totals t;
    int files = 0;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--corrupt")) { corrupt = true; continue; }
        std::vector<uint8_t> file;
        if (FILE *f = fopen(argv[a], "rb")) {
            uint8_t buf[4096];
            for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
            fclose(f);
        }
        std::string name = argv[a];
        name = name.substr(name.find_last_of('/') + 1);
        const Run base = run_walk(file);
        t.runs++;
        files++;
        if (corrupt) {
            t.nonzero += base.status != 0;
            if (base.reason || !base.ok || base.status == 0) {
                t.failures++;
                fprintf(stderr, "FAILED corrupt %s: reason %d status %d bounds %d\n", name.c_str(), base.reason, base.status, (int)base.ok);
            }
            continue;
        }
        if (base.reason) { t.refused++; continue; }   // (a stream the device does not take: nothing to walk)
        if (!base.ok || base.status != 0 || host_reader_fails(file)) {
            t.failures++;
            fprintf(stderr, "FAILED %s as it is: status %d bounds %d\n", name.c_str(), base.status, (int)base.ok);
            continue;
        }
        // truncation at every eighth byte
        for (size_t n = 8; n < file.size(); n += 8) {
            std::vector<uint8_t> v(file.begin(), file.begin() + n);
            check_variant("truncation", name, v, n, base, t);
        }
        // byte flips: one to three bytes, mostly inside the entropy-coded segment, some in the header and behind the data
        for (int k = 0; k < 48; k++) {
            std::vector<uint8_t> v = file;
            size_t first = v.size();
            const int nflip = 1 + (int)(rnd() % 3);
            for (int j = 0; j < nflip; j++) {
                size_t at = k % 8 == 7 ? rnd() % v.size() : base.ecs_off + rnd() % (v.size() - base.ecs_off);
                const uint8_t x = (uint8_t)(k % 3 == 0 ? 1u << (rnd() % 8) : 1 + rnd() % 255);
                v[at] ^= x;
                first = at < first ? at : first;
            }
            check_variant("byte flip", name, v, first, base, t);
        }
        // an early EOI, written over two bytes of the segment
        for (int k = 0; k < 8 && base.ecs_len > 4; k++) {
            std::vector<uint8_t> v = file;
            const size_t at = base.ecs_off + rnd() % (base.ecs_len - 1);
            v[at] = 0xFF; v[at + 1] = 0xD9;
            check_variant("early EOI", name, v, at, base, t);
        }
    }
    printf("{\"files\": %d, \"runs\": %ld, \"refused_by_parser\": %ld, \"nonzero_status\": %ld, \"host_reader_errors\": %ld, \"behind_last_read\": %ld, "
           "\"failures\": %ld}\n", files, t.runs, t.refused, t.nonzero, t.host_errors, t.behind, t.failures);
    return t.failures ? 1 : 0;
}
