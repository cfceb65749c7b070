// depth_fill.hip — REBVO's depth_filler (src/visualizer/depth_filler.cpp) for every sequence of a context: the dense inverse-depth grid
// the visualizer (visualizer.cpp:436-440) and the key-frame path (keyframe.cpp:171-184) interpolate from a KeyLine list.
//
// One workgroup per sequence runs the whole chain on the slot's SoA KeyLines, read only:
//   1. binning   each KeyLine that FillEdgeData (:113-163) would fold gets its cell; a count / scan / ordered scatter puts the KeyLine
//                ids of a cell into one bucket, in list order (stable: no sort, no dependence on the order the counting atomics took).
//   2. fusion    one lane per cell: ResetData's values (:41-56), then the information-form update for each KeyLine of its bucket, in order.
//   3. coarse-fine (InitCoarseFine, :233-297)  one lane per (level, tile) sums the tile in the reference's order (dx outer, dy inner);
//                then one lane per free cell takes the finest level whose tile around it holds a fixed cell.  A level reads only fixed
//                cells and the s_rho of boundary cells, which no level writes: the levels are independent of each other.
//   4. sweeps    iter_num x Integrate1Step (:301-355), in place, as a skewed wavefront: at step t every cell (x, y) of sweep k with
//                x + 2 y + 4 k = t updates.  Of its eight neighbours the four above / to the left were updated by sweep k at steps
//                t-3 .. t-1, the four below / to the right by sweep k-1 at steps t-3 .. t-1 and by sweep k not before t+1: exactly the
//                values the raster loop reads, in one buffer.  (With a skew of 3 sweep k+1 would reach (x-1, y-1) at the step at which
//                sweep k updates (x, y).)  No two cells of one step are neighbours.
// Three sources feed stages 1 and 2 (template parameter SRC of k_depth_fill; stages 3 and 4 are the same code for all; below NET is
// SRC == kDfNet and SEG is SRC == kDfSeg):
//   NET = false  the slot's SoA KeyLines with FillEdgeData(edge_tracker&, ...)'s gates (:113-163): the key-frame path's overload;
//   NET = true   a sequence's 15-byte wire records (net_keyline.hip) with FillEdgeData(net_keyline*, kn, p_off, ...)'s (:59-104): the
//                visualizer's overload (visualizer.cpp:436-439).  rho and s_rho come back from their 1 / NET_RHO_SCALING quanta, the cell from
//                (qx + p_off.x) / bl_size.w in float; there is no p_id / n_id / rho <= 0 gate and no rho0.
//   SEG          a sequence's decoded line segments (edgemap_decode.hip) as edgemap_com_decoder::fillDepthMap rasterises them
//                (src/CommLib/edgemap_com.cpp:475-528): what is binned and folded is a (segment, step) item, numbered by segment and
//                then by step — the order the reference's two nested loops update a cell in.  k_em_items has applied the gates and
//                scanned the step counts; an item finds its segment by bisection of those offsets, its cell by getImgPoint's unsigned
//                division and clamp (edgemap_seg.h), and folds rho = r1 * step + k0.rho with the segment's 1 / s_rho^2.
// The grid lives in LDS while it fits in 64 KB (rho, s_rho: 16 B per cell, fixed: 1 B — 3 600 cells at 10-px blocks of 752x480)
// and in the context's output arrays in HBM otherwise (14 400 cells at 5-px blocks); the code is the same on both.
// fp64 throughout; '/' and sqrt are the compiler's correctly rounded operations, the cell index uses its correctly rounded float
// division, and -ffp-contract=off keeps every product and sum separately rounded as in the reference.
#include "ctx.h"
#include "edgemap_seg.h"

#include <cmath>
#include <cstring>

namespace edgehip {

constexpr int kDfThreads = 512;
constexpr int kDfMaxLevels = 32;
constexpr size_t kDfLdsMax = 65536 - 4 * kDfThreads;   // dynamic LDS for the grid beside the scan's partials (64 KB: no opt-in)
constexpr double kRhoMax = 20.0;   // RHO_MAX, include/mtracklib/edge_finder.h:38

struct DfLevels {
    int nlev;
    int sx[kDfMaxLevels], sy[kDfMaxLevels], ntx[kDfMaxLevels], nty[kDfMaxLevels], base[kDfMaxLevels];
};

struct DfArgs {
    const KlSoA *kls;          // [nseq] KeyLines of the slot
    const int32_t *kns;        // [nseq]
    int32_t *cell;             // [nseq][cap] cell of each KeyLine, -1: not folded
    int32_t *cnt;              // [nseq][G] KeyLines per cell (zero between launches: the scatter counts them back down)
    int32_t *off;              // [nseq][G + 1] bucket offsets
    int32_t *ids;              // [nseq][cap] KeyLine ids by cell
    double *tile_r, *tile_s;   // [nseq][ntiles] mean_rho / mean_srho of every coarse-fine tile
    int32_t *tile_n;           // [nseq][ntiles] fixed cells of the tile
    double *rho, *s_rho;       // [nseq][G] the grids
    uint8_t *fixed;            // [nseq][G]
    int cap, gw, gh, bw, bh, iter_num, bound_mode, discard, m_num_t, ntiles;
    double v_thresh;
    int use_lds;
    // NET: the wire records instead of kls / kns
    const uint8_t *net_rec;              // [nseq][net_kl_size][15]
    const edgehip_net_header *net_hdr;   // [nseq]
    int net_kl_size;
    float p_off_x, p_off_y;
    // SEG: the decoded segments and their items instead of kls / kns (cap: cap_items; cell / ids: the decoder's)
    SegSource seg;
};
enum { kDfKeyLines = 0, kDfNet = 1, kDfSeg = 2 };

// the segment that owns item i: the last s with off[s] <= i (a segment without steps has off[s] == off[s + 1] and is passed over)
__device__ __forceinline__ int df_seg_of(const int32_t *off, int nseg, int i) {
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

constexpr double kNetRhoScale = 10000.0;   // NET_RHO_SCALING, include/CommLib/net_keypoint.h:32
// the fields FillEdgeData reads of wire record i (net_keyline: qx, qy, rho, s_rho at bytes 0 .. 7, m_num at byte 12), byte loads: a record is aligned to nothing
struct DfNetRec { int qx, qy, rho, s_rho, m_num; };
__device__ __forceinline__ DfNetRec df_net_rec(const uint8_t *rec, int i) {
    const uint8_t *p = rec + (size_t)i * 15;
    DfNetRec r;
    r.qx = ldg(p, 0) | (ldg(p, 1) << 8);
    r.qy = ldg(p, 2) | (ldg(p, 3) << 8);
    r.rho = ldg(p, 4) | (ldg(p, 5) << 8);
    r.s_rho = ldg(p, 6) | (ldg(p, 7) << 8);
    r.m_num = ldg(p, 12);
    return r;
}

// (uint) of a float as an x86-64 build converts it (cvttss2si to 64 bits, low 32 bits): what GetIndex receives (image.h:113)
__device__ __forceinline__ uint32_t x86_f2u(float q) {
    if (!(q > -9.2e18f && q < 9.2e18f)) return 0u;
    return (uint32_t)(long long)q;
}

__device__ __forceinline__ bool df_inboundary(int x, int y, int gw, int gh, int mode) {   // depth_filler::inboundary, :280-297
    if (mode == EDGEHIP_BOUND_CORNERS) return (x == 0 && (y == 0 || y == gh - 1)) || (x == gw - 1 && (y == 0 || y == gh - 1));
    if (mode == EDGEHIP_BOUND_FULL) return x == 0 || x == gw - 1 || y == 0 || y == gh - 1;
    return false;
}

template <int SRC>
__global__ __launch_bounds__(kDfThreads) void k_depth_fill(DfArgs a, DfLevels lv) {
    constexpr bool NET = SRC == kDfNet, SEG = SRC == kDfSeg;
    extern __shared__ __align__(16) unsigned char df_lds[];
    __shared__ int32_t part[kDfThreads];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int gw = a.gw, gh = a.gh, G = gw * gh;
    const KlSoA &k = a.kls[NET || SEG ? 0 : seq];   // (NET, SEG: not read)
    const int kn = SEG ? max(0, min(a.seg.items[seq], a.cap))
                       : NET ? max(0, min(min(a.net_hdr[seq].kline_num, a.net_kl_size), a.cap)) : min(a.kns[seq], a.cap);
    const int nseg = SEG ? max(0, min(a.seg.seg_num[seq], a.seg.cap_segments)) : 0;
    const float *sseg = SEG ? a.seg.seg + (size_t)seq * a.seg.cap_segments * 8 : nullptr;
    const int32_t *soff = SEG ? a.seg.seg_off + (size_t)seq * (a.seg.cap_segments + 1) : nullptr;
    const double *sdir = SEG ? a.seg.seg_dir + (size_t)seq * a.seg.cap_segments * 4 : nullptr;
    const uint8_t *nrec = NET ? a.net_rec + (size_t)seq * a.net_kl_size * 15 : nullptr;
    int32_t *cell = a.cell + (size_t)seq * a.cap;
    int32_t *cnt = a.cnt + (size_t)seq * G;
    int32_t *off = a.off + (size_t)seq * (G + 1);
    int32_t *ids = a.ids + (size_t)seq * a.cap;
    double *rho = a.rho + (size_t)seq * G, *s_rho = a.s_rho + (size_t)seq * G;
    uint8_t *fixed = a.fixed + (size_t)seq * G;
    double *g_rho = rho, *g_srho = s_rho;
    uint8_t *g_fixed = fixed;
    if (a.use_lds) {
        g_rho = (double *)df_lds;
        g_srho = g_rho + G;
        g_fixed = (uint8_t *)(g_srho + G);
    }

    // 1. cells (FillEdgeData's tests, in its order) and counts
    for (int i = tid; i < kn; i += kDfThreads) {
        int c = -1;
        if constexpr (SEG) {   // (kn > 0 only with nseg > 0; every item has a cell: getImgPoint clamps into the grid)
            const int sg = df_seg_of(soff, nseg, i);
            rebvo::edgemap::SegSteps st;
            st.q0x = sseg[8 * sg]; st.q0y = sseg[8 * sg + 1];
            st.tx = sdir[4 * sg]; st.ty = sdir[4 * sg + 1];
            c = rebvo::edgemap::seg_step_cell(st, i - soff[sg], a.bw, a.bh, gw, gh);
            cell[i] = c;
            atomicAdd(&cnt[c], 1);
            continue;
        }
        if constexpr (NET) {
            const DfNetRec n = df_net_rec(nrec, i);
            const double r = n.rho / kNetRhoScale, s = n.s_rho / kNetRhoScale;
            if (!(s / r > a.v_thresh) && !(n.m_num < a.m_num_t && a.discard)) {
                // (nkl.qx + p_off.x) / bl_size.w: u_short -> int -> float, float sum, float quotient by the u_int block size
                const uint32_t idx = x86_f2u(((float)n.qy + a.p_off_y) / (float)a.bh) * (uint32_t)gw + x86_f2u(((float)n.qx + a.p_off_x) / (float)a.bw);
                if (idx < (uint32_t)G) c = (int)idx;   // past the last cell: dropped, as below
            }
            cell[i] = c;
            if (c >= 0) atomicAdd(&cnt[c], 1);
            continue;
        }
        const double r = ldg(k.rho, i), s = ldg(k.s_rho, i);
        if (!(s / r > a.v_thresh)) {
            const bool weak = ldg(k.m_num, i) < a.m_num_t || ldg(k.p_id, i) < 0 || ldg(k.n_id, i) < 0 || r <= 0;
            if (!(weak && a.discard)) {
                const float2 cp = ldg(k.c_p, i);
                const uint32_t idx = x86_f2u(cp.y / (float)a.bh) * (uint32_t)gw + x86_f2u(cp.x / (float)a.bw);
                if (idx < (uint32_t)G) c = (int)idx;   // past the last cell: the reference writes out of bounds there (dropped)
            }
        }
        cell[i] = c;
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();

    // exclusive scan of the counts: a contiguous run of cells per thread, then the 512 run totals
    const int run = (G + kDfThreads - 1) / kDfThreads;
    const int c0 = min(G, tid * run), c1 = min(G, c0 + run);
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += cnt[c];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kDfThreads; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int o = part[tid] - sum;
    for (int c = c0; c < c1; c++) { off[c] = o; o += cnt[c]; }
    if (tid == kDfThreads - 1) off[G] = part[tid];
    __syncthreads();

    // scatter in list order: wave 0 walks the list 64 KeyLines at a time.  The first lane of each cell in the chunk takes the chunk's share
    // of the bucket with one atomicSub on the count of places still free (its result is used before the next chunk's atomic is issued, so
    // the chunks claim their places in list order); a lane's place is then that share plus the number of lower lanes with the same cell.
    // The counts end at zero, ready for the next launch.  No sort: the buckets come out in list order.
    if (tid < warpSize) {
        for (int i0 = 0; i0 < kn; i0 += warpSize) {
            const int i = i0 + tid;
            const int c = i < kn ? cell[i] : -1;
            int rank = 0, same = 0, first = warpSize;
            for (int j = 0; j < warpSize; j++) {
                const int cj = __shfl(c, j);
                if (c >= 0 && cj == c) {
                    same++;
                    if (j < tid) rank++;
                    first = min(first, j);
                }
            }
            const int left = (c >= 0 && rank == 0) ? atomicSub(&cnt[c], same) : 0;   // places of the bucket not yet taken
            const int base = __shfl(left, first < warpSize ? first : 0);
            if (c >= 0) ids[off[c + 1] - base + rank] = i;
        }
    }
    __syncthreads();

    // 2. ResetData + the fold of each cell's KeyLines in list order
    for (int c = tid; c < G; c += kDfThreads) {
        const int b0 = off[c], b1 = off[c + 1];
        double cr = 1.0, cs = kRhoMax * 2, I = 1.0 / ((kRhoMax * 2) * (kRhoMax * 2));
        for (int j = b0; j < b1; j++) {
            const int i = ids[j];
            double r, kl_I;
            if constexpr (SEG) {
                const int sg = df_seg_of(soff, nseg, i);
                rebvo::edgemap::SegSteps st;
                st.r1 = sdir[4 * sg + 2]; st.rho0 = sseg[8 * sg + 2];
                r = rebvo::edgemap::seg_step_rho(st, i - soff[sg]);
                kl_I = sdir[4 * sg + 3];   // (the update below is the one loop all three sources share; seg_fold is the host's copy of it)
            } else if constexpr (NET) {
                const DfNetRec n = df_net_rec(nrec, i);
                r = n.rho / kNetRhoScale;
                double s = n.s_rho / kNetRhoScale;
                if (n.m_num < a.m_num_t) s = kRhoMax;   // (discard: such a record got no cell)
                kl_I = 1 / (s * s);
            } else {
                r = ldg(k.rho, i);
                const double s = ldg(k.s_rho, i);
                kl_I = 1.0 / (s * s);
                if (ldg(k.m_num, i) < a.m_num_t || ldg(k.p_id, i) < 0 || ldg(k.n_id, i) < 0 || r <= 0) {
                    kl_I = 1.0 / (kRhoMax * kRhoMax);
                    if (r < 0) r = ldg(k.rho0, i);   // (the reference writes this back into the KeyLine; the device only reads)
                }
            }
            double i_rho = I * cr;
            i_rho += r * kl_I;
            I += kl_I;
            const double v = I > 0 ? 1.0 / I : 1e20;
            cr = i_rho * v;
            cs = sqrt(v);
        }
        g_rho[c] = cr;
        g_srho[c] = cs;
        g_fixed[c] = b1 > b0;
    }
    __syncthreads();

    // 3. coarse-fine: every tile of every level
    double *tr = a.tile_r + (size_t)seq * a.ntiles, *ts = a.tile_s + (size_t)seq * a.ntiles;
    int32_t *tn = a.tile_n + (size_t)seq * a.ntiles;
    for (int j = tid; j < a.ntiles; j += kDfThreads) {
        int l = 0;
        while (l + 1 < lv.nlev && j >= lv.base[l + 1]) l++;
        const int sx = lv.sx[l], sy = lv.sy[l], t = j - lv.base[l];
        const int x = (t % lv.ntx[l]) * sx, y = (t / lv.ntx[l]) * sy;
        double mr = 0, ms = 0;
        int n = 0, nr = 0;
        for (int dx = 0; dx < sx; dx++)
            for (int dy = 0; dy < sy; dy++) {
                const int c = (y + dy) * gw + x + dx;
                if (g_fixed[c]) {
                    mr += g_rho[c];
                    ms += g_srho[c];
                    n++;
                    nr++;
                } else if (df_inboundary(x + dx, y + dy, gw, gh, a.bound_mode)) {
                    ms += g_srho[c];
                    nr++;
                }
            }
        if (n > 0) {
            mr /= n;
            ms /= nr;
        }
        tr[j] = mr;
        ts[j] = ms;
        tn[j] = n;
    }
    __syncthreads();
    for (int c = tid; c < G; c += kDfThreads) {
        if (g_fixed[c]) continue;
        const int x = c % gw, y = c / gw;
        for (int l = lv.nlev - 1; l >= 0; l--) {
            const int tx = x / lv.sx[l], ty = y / lv.sy[l];
            if (tx >= lv.ntx[l] || ty >= lv.nty[l]) continue;
            const int j = lv.base[l] + ty * lv.ntx[l] + tx;
            if (tn[j] > 0) {
                g_rho[c] = tr[j];
                if (!df_inboundary(x, y, gw, gh, a.bound_mode)) g_srho[c] = ts[j];
                break;
            }
        }
    }
    __syncthreads();

    // 4. the Gauss-Seidel sweeps on the wavefront t = x + 2 y + 4 k
    if (a.iter_num > 0) {
        const int T = (gw - 1) + 2 * (gh - 1) + 4 * (a.iter_num - 1) + 1;
        const int items = a.iter_num * gh;
        for (int t = 0; t < T; t++) {
            for (int q = tid; q < items; q += kDfThreads) {
                const int kk = q / gh, y = q - kk * gh;
                const int x = t - 4 * kk - 2 * y;
                if (x < 0 || x >= gw) continue;
                const int c = y * gw + x;
                if (g_fixed[c]) continue;
                double r = 0, sr = 0;
                int n = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if (dx == 0 && dy == 0) continue;
                        const int px = x + dx, py = y + dy;
                        if (px < 0 || px >= gw || py < 0 || py >= gh) continue;
                        r += g_rho[py * gw + px];
                        sr += g_srho[py * gw + px];
                        n++;
                    }
                const double w = 1.0;
                g_rho[c] = (1 - w) * g_rho[c] + w * r / n;   // (1 - w) * rho: -0 for a negative rho, NaN for a non-finite one
                if (!df_inboundary(x, y, gw, gh, a.bound_mode)) g_srho[c] = sr / n;
            }
            __syncthreads();
        }
    }

    if (a.use_lds) {
        for (int c = tid; c < G; c += kDfThreads) {
            rho[c] = g_rho[c];
            s_rho[c] = g_srho[c];
            fixed[c] = g_fixed[c];
        }
    }
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::DepthFill {
    edgehip_depth_fill_params p;
    int gw, gh;
    DfLevels lv;
    int ntiles;
    bool use_lds;
    void *arena = nullptr;
    int32_t *cell, *cnt, *off, *ids, *tile_n;
    double *tile_r, *tile_s, *rho, *s_rho;
    uint8_t *fixed;
    bool filled = false;   // an edgehip_depth_fill / edgehip_depth_fill_net was enqueued since the enable
    // edgehip_depth_fill_net with more records per sequence than the KeyLine capacity: cell / ids of its own (grown, never shrunk)
    int32_t *net_scratch = nullptr;
    int net_scratch_cap = 0;
};

static void depth_fill_release(edgehip_ctx *c) {
    if (!c->dfill) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->dfill->arena) (void)hipFree(c->dfill->arena);
    if (c->dfill->net_scratch) (void)hipFree(c->dfill->net_scratch);
    delete c->dfill;
    c->dfill = nullptr;
}

void edgehip::depth_fill_free(edgehip_ctx *c) {
    depth_surface_free(c);
    surface_views_free(c);
    depth_fill_release(c);
}

int edgehip::depth_fill_geometry(edgehip_ctx *c, int32_t *gw, int32_t *gh, int32_t *bw, int32_t *bh) {
    if (!c->dfill) return EDGEHIP_ERR_STATE;
    *gw = c->dfill->gw; *gh = c->dfill->gh; *bw = c->dfill->p.block_w; *bh = c->dfill->p.block_h;
    return 0;
}

bool edgehip::depth_fill_grids(edgehip_ctx *c, const double **rho, const double **s_rho) {
    if (!c->dfill || !c->dfill->filled) return false;
    *rho = c->dfill->rho;
    *s_rho = c->dfill->s_rho;
    return true;
}

int edgehip_depth_fill_enable(edgehip_ctx *c, const edgehip_depth_fill_params *p) {
    EH_ENTER(c);
    if (!p) { depth_fill_free(c); return 0; }
    if (p->block_w < 1 || p->block_h < 1 || p->iter_num < 0 || p->bound_mode < EDGEHIP_BOUND_NONE || p->bound_mode > EDGEHIP_BOUND_FULL) {
        set_error("depth_fill_enable: block sizes must be >= 1, iter_num >= 0, bound_mode one of EDGEHIP_BOUND_*");
        return EDGEHIP_ERR_ARG;
    }
    const int gw = c->plan.w / p->block_w, gh = c->plan.h / p->block_h;
    if (gw < 1 || gh < 1) { set_error("depth_fill_enable: the grid (image size / block size) is smaller than 1x1"); return EDGEHIP_ERR_ARG; }
    // the depth surface stays enabled while the blocks (and so the grid) stay the same; it reads the new grids after the next fill
    if (c->dfill && (c->dfill->p.block_w != p->block_w || c->dfill->p.block_h != p->block_h)) { depth_surface_free(c); surface_views_free(c); }
    depth_fill_release(c);
    auto *d = new edgehip_ctx::DepthFill;
    d->p = *p;
    d->gw = gw;
    d->gh = gh;
    memset(&d->lv, 0, sizeof d->lv);
    int nt = 0;
    for (int sx = gw, sy = gh; sx > 1 && sy > 1; sx /= 2, sy /= 2) {   // InitCoarseFine's levels (depth_filler.cpp:236)
        const int l = d->lv.nlev++;
        d->lv.sx[l] = sx; d->lv.sy[l] = sy;
        d->lv.ntx[l] = (gw - sx) / sx + 1; d->lv.nty[l] = (gh - sy) / sy + 1;
        d->lv.base[l] = nt;
        nt += d->lv.ntx[l] * d->lv.nty[l];
    }
    d->ntiles = nt;
    const size_t B = c->plan.nseq, G = (size_t)gw * gh, cap = c->plan.cap, T = (size_t)std::max(nt, 1);
    d->use_lds = G * 17 <= kDfLdsMax;
    // one allocation: the doubles first (8-byte aligned), then the 4-byte and 1-byte arrays
    const size_t n_dbl = B * (2 * G + 2 * T), n_i32 = B * (2 * cap + 2 * G + 1 + T), n_u8 = B * G;
    const size_t bytes = 8 * n_dbl + 4 * n_i32 + n_u8;
    if (hipMalloc(&d->arena, bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete d;
        depth_surface_free(c);
        surface_views_free(c);
        set_error("depth_fill_enable: device allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    char *q = (char *)d->arena;
    d->rho = (double *)q; q += 8 * B * G;
    d->s_rho = (double *)q; q += 8 * B * G;
    d->tile_r = (double *)q; q += 8 * B * T;
    d->tile_s = (double *)q; q += 8 * B * T;
    d->cell = (int32_t *)q; q += 4 * B * cap;
    d->ids = (int32_t *)q; q += 4 * B * cap;
    d->cnt = (int32_t *)q; q += 4 * B * G;
    d->off = (int32_t *)q; q += 4 * B * (G + 1);
    d->tile_n = (int32_t *)q; q += 4 * B * T;
    d->fixed = (uint8_t *)q;
    // the counts must start at zero; the grids read as empty before a fill.  The fill is published only once that is enqueued.
    if (hipMemsetAsync(d->arena, 0, bytes, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d->arena);
        delete d;
        depth_surface_free(c);
        surface_views_free(c);
        set_error("depth_fill_enable: hipMemsetAsync failed");
        return EDGEHIP_ERR_DEVICE;
    }
    c->dfill = d;
    return 0;
}

int edgehip_depth_fill_size(edgehip_ctx *c, int32_t *gw, int32_t *gh) {
    EH_ENTER(c);
    if (!c->dfill) { set_error("depth_fill_size: depth fill is not enabled"); return EDGEHIP_ERR_STATE; }
    if (!gw || !gh) { set_error("depth_fill_size: null argument"); return EDGEHIP_ERR_ARG; }
    *gw = c->dfill->gw;
    *gh = c->dfill->gh;
    return 0;
}

int edgehip_depth_fill(edgehip_ctx *c, int slot) {
    EH_ENTER(c);
    if (slot < 0 || slot >= c->plan.nslots) { set_error("depth_fill: slot out of range"); return EDGEHIP_ERR_ARG; }
    auto *d = c->dfill;
    if (!d) { set_error("depth_fill: depth fill is not enabled (edgehip_depth_fill_enable)"); return EDGEHIP_ERR_STATE; }
    // the slot's KeyLines as edgehip_download_keylines returns them: the turned rho / s_rho of an OLD slot the frame driver keeps
    // beside the slot's arrays come in first (ctx.h, fuse_match), and the slot's stage A on the other stream is ordered before
    if (int e = rot_materialize_enqueue(c, slot)) return e;
    if (int e = order_bc_after_a(c)) return e;
    DfArgs a;
    a.kls = kldev(c, slot);
    a.kns = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.cell = d->cell; a.cnt = d->cnt; a.off = d->off; a.ids = d->ids;
    a.tile_r = d->tile_r; a.tile_s = d->tile_s; a.tile_n = d->tile_n;
    a.rho = d->rho; a.s_rho = d->s_rho; a.fixed = d->fixed;
    a.cap = c->plan.cap; a.gw = d->gw; a.gh = d->gh; a.bw = d->p.block_w; a.bh = d->p.block_h;
    a.iter_num = d->p.iter_num; a.bound_mode = d->p.bound_mode; a.discard = d->p.discard != 0; a.m_num_t = d->p.thresh_match_num;
    a.ntiles = d->ntiles; a.v_thresh = d->p.thresh_rel_rho; a.use_lds = d->use_lds;
    const size_t lds = d->use_lds ? (size_t)d->gw * d->gh * 17 : 0;
    a.net_rec = nullptr; a.net_hdr = nullptr; a.net_kl_size = 0; a.p_off_x = a.p_off_y = 0.f;
    a.seg = SegSource{};
    hipLaunchKernelGGL(k_depth_fill<kDfKeyLines>, dim3(c->plan.nseq), dim3(kDfThreads), lds, c->stream, a, d->lv);
    EH_LAUNCH_CHECK();
    d->filled = true;
    return slot_read_done(c, slot);   // a later stage A that detects into this slot waits for the fill's reads
}

int edgehip_depth_fill_net(edgehip_ctx *c, float p_off_x, float p_off_y) {
    EH_ENTER(c);
    auto *d = c->dfill;
    if (!d) { set_error("depth_fill_net: depth fill is not enabled (edgehip_depth_fill_enable)"); return EDGEHIP_ERR_STATE; }
    DfArgs a;
    if (!net_store(c, &a.net_rec, &a.net_hdr, &a.net_kl_size)) { set_error("depth_fill_net: the record store is not enabled (edgehip_net_enable)"); return EDGEHIP_ERR_STATE; }
    a.cell = d->cell; a.ids = d->ids; a.cap = c->plan.cap;
    if (a.net_kl_size > c->plan.cap) {   // more records than KeyLines fit: binning scratch of that size
        const size_t B = c->plan.nseq;
        if (d->net_scratch_cap < a.net_kl_size) {
            EH_CHECK(hipStreamSynchronize(c->stream));
            if (d->net_scratch) { (void)hipFree(d->net_scratch); d->net_scratch = nullptr; d->net_scratch_cap = 0; }
            void *q = nullptr;
            if (hipMalloc(&q, 4 * 2 * B * (size_t)a.net_kl_size) != hipSuccess) { (void)hipGetLastError(); set_error("depth_fill_net: device allocation failed"); return EDGEHIP_ERR_MEMORY; }
            d->net_scratch = (int32_t *)q;
            d->net_scratch_cap = a.net_kl_size;
        }
        a.cap = d->net_scratch_cap;
        a.cell = d->net_scratch;
        a.ids = d->net_scratch + B * (size_t)a.cap;
    }
    a.kls = kldev(c, 0); a.kns = c->kn_slot;   // not read
    a.cnt = d->cnt; a.off = d->off;
    a.tile_r = d->tile_r; a.tile_s = d->tile_s; a.tile_n = d->tile_n;
    a.rho = d->rho; a.s_rho = d->s_rho; a.fixed = d->fixed;
    a.gw = d->gw; a.gh = d->gh; a.bw = d->p.block_w; a.bh = d->p.block_h;
    a.iter_num = d->p.iter_num; a.bound_mode = d->p.bound_mode; a.discard = d->p.discard != 0; a.m_num_t = d->p.thresh_match_num;
    a.ntiles = d->ntiles; a.v_thresh = d->p.thresh_rel_rho; a.use_lds = d->use_lds;
    a.p_off_x = p_off_x; a.p_off_y = p_off_y;
    a.seg = SegSource{};
    const size_t lds = d->use_lds ? (size_t)d->gw * d->gh * 17 : 0;
    hipLaunchKernelGGL(k_depth_fill<kDfNet>, dim3(c->plan.nseq), dim3(kDfThreads), lds, c->stream, a, d->lv);
    EH_LAUNCH_CHECK();
    d->filled = true;
    return 0;
}

int edgehip_depth_fill_segments(edgehip_ctx *c, double v_thresh, double a_thresh_deg, int use_visibility) {
    EH_ENTER(c);
    auto *d = c->dfill;
    if (!d) { set_error("depth_fill_segments: depth fill is not enabled (edgehip_depth_fill_enable)"); return EDGEHIP_ERR_STATE; }
    if (std::isnan(v_thresh) || std::isnan(a_thresh_deg)) { set_error("depth_fill_segments: NaN threshold"); return EDGEHIP_ERR_ARG; }
    DfArgs a;
    if (int e = edgemap_items_enqueue(c, v_thresh, a_thresh_deg, use_visibility, &a.seg)) return e;
    a.kls = kldev(c, 0); a.kns = c->kn_slot;   // not read
    a.cell = a.seg.cell; a.ids = a.seg.ids; a.cap = a.seg.cap_items;
    a.cnt = d->cnt; a.off = d->off;
    a.tile_r = d->tile_r; a.tile_s = d->tile_s; a.tile_n = d->tile_n;
    a.rho = d->rho; a.s_rho = d->s_rho; a.fixed = d->fixed;
    a.gw = d->gw; a.gh = d->gh; a.bw = d->p.block_w; a.bh = d->p.block_h;
    a.iter_num = d->p.iter_num; a.bound_mode = d->p.bound_mode; a.discard = 0; a.m_num_t = 0;
    a.ntiles = d->ntiles; a.v_thresh = v_thresh; a.use_lds = d->use_lds;
    a.net_rec = nullptr; a.net_hdr = nullptr; a.net_kl_size = 0; a.p_off_x = a.p_off_y = 0.f;
    const size_t lds = d->use_lds ? (size_t)d->gw * d->gh * 17 : 0;
    edgemap_decode_mark(c, 3, false);
    hipLaunchKernelGGL(k_depth_fill<kDfSeg>, dim3(c->plan.nseq), dim3(kDfThreads), lds, c->stream, a, d->lv);
    edgemap_decode_mark(c, 3, true);
    EH_LAUNCH_CHECK();
    d->filled = true;
    return 0;
}

int edgehip_download_depth_grids_batch(edgehip_ctx *c, int n, const int32_t *seqs, double *const *rho, double *const *s_rho,
                                       uint8_t *const *fixed) {
    EH_ENTER(c);
    auto *d = c->dfill;
    if (!d) { set_error("download_depth_grid: depth fill is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_depth_grid: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_depth_grid: sequence out of range"); return EDGEHIP_ERR_ARG; }
    const size_t G = (size_t)d->gw * d->gh;
    for (int j = 0; j < n; j++) {
        const size_t o = (size_t)seqs[j] * G;
        if (rho && rho[j]) EH_CHECK(hipMemcpyAsync(rho[j], d->rho + o, 8 * G, hipMemcpyDeviceToHost, c->stream));
        if (s_rho && s_rho[j]) EH_CHECK(hipMemcpyAsync(s_rho[j], d->s_rho + o, 8 * G, hipMemcpyDeviceToHost, c->stream));
        if (fixed && fixed[j]) EH_CHECK(hipMemcpyAsync(fixed[j], d->fixed + o, G, hipMemcpyDeviceToHost, c->stream));
    }
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_depth_grid(edgehip_ctx *c, int seq, double *rho, double *s_rho, uint8_t *fixed) {
    return edgehip_download_depth_grids_batch(c, 1, &seq, &rho, &s_rho, &fixed);
}
