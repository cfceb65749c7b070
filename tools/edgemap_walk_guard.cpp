// Guard of the compressed edge map's walk (rebvo_amd/csrc/edgemap_fit.h) on seeded random link graphs, a stand-alone CPU program: build
// it with -fsanitize=address,undefined and run it (tests/test_edgemap_cpu.py does).
//
// Graphs: random n_id with merges (several KeyLines naming one successor), cycles, self-links and links outside [-1, kn); p_id written
// last-writer from the in-range n_id, as edge_finder::join_edges leaves it, now and then an out-of-range one; random depths.
// Checked, per graph:
//   - the component-wise execution the device runs (components of the n_id graph by minimum index, one component after the other in a
//     SHUFFLED order, its heads ascending; a counting pass, a scan in index order, a fitting pass) gives the records of the straight
//     serial loop rebvo_compress_edgemap, byte for byte, and the same count and status;
//   - every KeyLine index any accessor sees is inside [0, kn), every mask index likewise, every record index inside the span;
//   - canary bands around the record spans and the masks are intact;
//   - no walk reaches its step bound (kStepGuard never set), and no walk asks for more than kn + 1 successors outside its fits;
//   - a span that is too small gives count 0 and kOverflow in both executions.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "rebvo/edgemap_com.h"

using namespace rebvo::edgemap;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) { fprintf(stderr, "edgemap_walk_guard: %s failed (line %d, seed %u)\n", #c, __LINE__, g_seed); exit(1); } \
    } while (0)
static unsigned g_seed = 0;
static long g_records = 0, g_fitted = 0, g_bad_link_graphs = 0, g_heads = 0;

constexpr int kBand = 64;
constexpr uint8_t kCanary = 0xA5;

struct GuardedKeyLines {   // AosKeyLines with every index checked
    AosKeyLines a;
    mutable long nexts = 0;
    void in(int k) const { CHECK(k >= 0 && k < a.n); }
    int kn() const { return a.n; }
    int next(int k) const { in(k); nexts++; const int v = a.next(k); CHECK(v >= -1 && v < a.n); return v; }
    int prev(int k) const { in(k); const int v = a.prev(k); CHECK(v >= -1 && v < a.n); return v; }
    float cx(int k) const { in(k); return a.cx(k); }
    float cy(int k) const { in(k); return a.cy(k); }
    float ux(int k) const { in(k); return a.ux(k); }
    float uy(int k) const { in(k); return a.uy(k); }
    double rho(int k) const { in(k); return a.rho(k); }
    double s_rho(int k) const { in(k); return a.s_rho(k); }
    int m_num(int k) const { in(k); return a.m_num(k); }
};
struct GuardedMask {
    uint8_t *m;
    int n;
    bool get(int k) const { CHECK(k >= 0 && k < n); return m[k] != 0; }
    void set(int k) { CHECK(k >= 0 && k < n); m[k] = 1; }
    void clear(int k) { CHECK(k >= 0 && k < n); m[k] = 0; }
};
struct GuardedOut {
    enum { kFit = 1 };
    compressed_kl *out;
    int base, end;         // the head's own span [base, end)
    void put(int i, const Rec &r) {
        CHECK(i >= 0 && base + i < end);
        out[base + i].x = r.x; out[base + i].y = r.y; out[base + i].rho = r.rho; out[base + i].s_rho = r.s_rho;
    }
};

template <class T> struct Banded {   // n elements between two canary bands
    std::vector<uint8_t> raw;
    size_t n;
    explicit Banded(size_t n_) : raw(2 * kBand + n_ * sizeof(T), kCanary), n(n_) { memset(raw.data() + kBand, 0, n * sizeof(T)); }
    T *data() { return (T *)(raw.data() + kBand); }
    bool intact() const {
        for (int i = 0; i < kBand; i++)
            if (raw[i] != kCanary || raw[raw.size() - 1 - i] != kCanary) return false;
        return true;
    }
};

static std::vector<edgehip_keyline> random_graph(std::mt19937 &g, int kn) {
    std::vector<edgehip_keyline> kl((size_t)kn + 1);
    memset(kl.data(), 0, sizeof(edgehip_keyline) * kl.size());
    std::uniform_real_distribution<double> u(0, 1);
    const int shape = g() % 4;   // 0: mostly chains, 1: many merges, 2: random, 3: hostile links
    for (int k = 0; k < kn; k++) {
        edgehip_keyline &q = kl[k];
        const double a = u(g) * 6.283185307179586;
        q.c_p[0] = (float)(u(g) * 752); q.c_p[1] = (float)(u(g) * 480);
        q.u_m[0] = (float)cos(a); q.u_m[1] = (float)sin(a);
        q.rho = 0.2 + 2.8 * u(g);
        q.s_rho = 0.01 + u(g) * (g() % 3 ? 0.2 : 3.0);
        q.m_num = (int)(g() % 5);
        q.p_id = -1;
        const double r = u(g);
        int n = -1;
        if (shape == 0) n = r < 0.9 ? k + 1 : (r < 0.95 ? -1 : (int)(g() % kn));
        else if (shape == 1) n = r < 0.5 ? k + 1 : (r < 0.9 ? (int)(g() % (kn < 8 ? kn : 8)) * (kn / 8 > 0 ? kn / 8 : 1) : -1);
        else if (shape == 2) n = r < 0.8 ? (int)(g() % kn) : (r < 0.9 ? k : -1);
        else n = r < 0.6 ? (int)(g() % kn) : (r < 0.7 ? k : (r < 0.8 ? kn + (int)(g() % 5) : (r < 0.85 ? -2 - (int)(g() % 9) : (r < 0.9 ? 2147483647 : -1))));
        q.n_id = n;
    }
    for (int k = 0; k < kn; k++)
        if (kl[k].n_id >= 0 && kl[k].n_id < kn) kl[kl[k].n_id].p_id = k;
    if (shape == 3)
        for (int k = 0; k < kn; k += 7) kl[k].p_id = (k % 14) ? kn + 3 : -9;
    // a run of near-collinear KeyLines with consistent depth now and then, so that non-degenerate fits occur
    if (kn > 12 && shape < 2) {
        const int s = (int)(g() % (kn - 12));
        for (int i = 0; i < 12; i++) {
            edgehip_keyline &q = kl[s + i];
            q.c_p[0] = 100.f + 2.f * i; q.c_p[1] = 80.f + 1.f * i;
            q.u_m[0] = -0.4472136f; q.u_m[1] = 0.8944272f;
            q.rho = 1.0 + 0.002 * i; q.s_rho = 0.05; q.m_num = 4;
        }
    }
    return kl;
}

static int find_root(std::vector<int> &lab, int i) {
    while (lab[i] != i) i = lab[i] = lab[lab[i]];
    return i;
}

static void one_graph(unsigned seed) {
    g_seed = seed;
    std::mt19937 g(seed);
    const int kn = (int)(g() % 301);
    const std::vector<edgehip_keyline> kl = random_graph(g, kn);
    edgehip_edgemap_params p = {};
    p.min_line_len = (int)(g() % 4);
    p.max_line_len = 1 + (int)(g() % 24);
    p.match_n_t = (int)(g() % 4);
    p.max_angle = 0.1 + 1.2 * (g() % 100) / 100.0;
    p.rho_rel_max = (g() % 2) ? 1.3 : 4.0;
    const double scale = 0.5 + (g() % 4);
    const float ppx = 367.215f, ppy = 248.375f;
    const double zfm = 457.975;
    const int cap = 4 * kn + 4;

    // the straight serial loop
    Banded<compressed_kl> serial((size_t)cap);
    int st_serial = 0;
    const int n_serial = rebvo_compress_edgemap(kl.data(), kn, p, scale, ppx, ppy, zfm, serial.data(), cap, &st_serial);
    CHECK(n_serial >= 0 && n_serial <= cap && serial.intact());
    CHECK(!(st_serial & (kStepGuard | kOverflow)));

    // the component-wise execution
    const WalkParams w = walk_params(p, scale, ppx, ppy, zfm);
    GuardedKeyLines acc = {{kl.data(), kn}};
    int st = 0;
    std::vector<int> lab((size_t)kn + 1);
    std::iota(lab.begin(), lab.end(), 0);
    for (int k = 0; k < kn; k++) {
        if (link_is_bad(kl[k].n_id, kn) || link_is_bad(kl[k].p_id, kn)) st |= kBadLink;
        const int n = link_in_range(kl[k].n_id, kn);
        if (n < 0) continue;
        const int a = find_root(lab, k), b = find_root(lab, n);
        if (a != b) lab[a > b ? a : b] = a > b ? b : a;   // the minimum index labels the component
    }
    std::vector<std::vector<int>> heads((size_t)kn + 1);   // per label, ascending
    std::vector<int> comps;
    for (int k = 0; k < kn; k++) {
        if (acc.prev(k) >= 0) continue;
        const int r = find_root(lab, k);
        CHECK(r <= k);
        if (heads[r].empty()) comps.push_back(r);
        heads[r].push_back(k);
    }
    std::shuffle(comps.begin(), comps.end(), g);
    std::vector<int> offs((size_t)kn + 1, 0), cnt((size_t)kn + 1, 0);
    Banded<uint8_t> m1((size_t)kn), m2((size_t)kn);
    GuardedMask mask = {m1.data(), kn};
    for (int r : comps)
        for (int h : heads[r]) {
            if (mask.get(h)) continue;
            CountOnly o;
            const long before = acc.nexts;
            cnt[h] = walk_head(acc, mask, w, h, o, st);
            CHECK(acc.nexts - before <= 2L * kn + 3);   // <= kn + 1 steps, and the unmasking walks at most the path again
        }
    int total = 0;
    for (int k = 0; k < kn; k++) { offs[k] = total; total += cnt[k]; }
    CHECK(total == n_serial);
    Banded<compressed_kl> par((size_t)cap);
    std::shuffle(comps.begin(), comps.end(), g);
    mask = GuardedMask{m2.data(), kn};
    for (int r : comps)
        for (int h : heads[r]) {
            if (mask.get(h)) continue;
            GuardedOut o = {par.data(), offs[h], offs[h] + cnt[h]};
            CHECK(walk_head(acc, mask, w, h, o, st) == cnt[h]);
        }
    CHECK(!(st & kStepGuard));
    CHECK(st == st_serial);
    CHECK(par.intact() && m1.intact() && m2.intact());
    CHECK(memcmp(par.data(), serial.data(), sizeof(compressed_kl) * (size_t)n_serial) == 0);
    g_records += n_serial;
    for (int i = 0; i < n_serial; i++) g_fitted += serial.data()[i].s_rho < 255;
    g_bad_link_graphs += (st & kBadLink) != 0;
    for (int r : comps) g_heads += (long)heads[r].size();

    // a span one record too small
    if (n_serial > 0) {
        Banded<compressed_kl> small((size_t)n_serial - 1);
        int st2 = 0;
        CHECK(rebvo_compress_edgemap(kl.data(), kn, p, scale, ppx, ppy, zfm, small.data(), n_serial - 1, &st2) == 0);
        CHECK((st2 & kOverflow) && small.intact());
    }
}

int main(int argc, char **argv) {
    const int graphs = argc > 1 ? atoi(argv[1]) : 400;
    for (int i = 0; i < graphs; i++) one_graph(1000u + (unsigned)i);
    CHECK(g_records > 0 && g_fitted > 0 && g_bad_link_graphs > 0);   // the graphs are not all trivial
    printf("edgemap_walk_guard: %d graphs ok (%ld heads, %ld records, %ld of them with a fitted sigma, %ld graphs with links out of range)\n", graphs,
           g_heads, g_records, g_fitted, g_bad_link_graphs);
    return 0;
}
