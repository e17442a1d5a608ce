// Cloud-in-cell (order 2) and triangular-shaped-cloud (order 3) mass assignment on periodic boxes, 2-D and 3-D, in the two forms of the
// NGP deposit (bfgx_deposit.hpp): one thread per particle with global fp64 atomics, and the tile-owned form.  The orders are those of
// engine.WINDOW_ORDERS, so the window that cross_power_spectrum divides out is the one deposited here.
//
// Per axis (grid of N cells on [0, L], s = N / L, t = v s rounded once):
//   dropped   !(0 <= v <= L): below, above, NaN, +-inf; the whole particle goes (np.histogramdd's rule; v == L and -0.0 are inside)
//   CIC       u = t - 0.5, i = floor(u), f = u - i: cell i mod N gets 1 - f, cell (i + 1) mod N gets f (i = -1 for u < 0)
//   TSC       i = min(floor(t), N - 1), d = t - i - 0.5: cells (i - 1) mod N, i, (i + 1) mod N get 0.5 (0.5 - d)^2, 0.75 - d^2, 0.5 (0.5 + d)^2
// On the SHIFTED grid (template flag SHIFT: grid 2 of an interlaced pair, every particle moved by +L / (2N) along every axis, periodically;
// which particles are kept does not change, v == L lands in cell 0):
//   CIC       i = floor(t) (0 .. N), f = t - i: cells i mod N and (i + 1) mod N get 1 - f and f
//   TSC       t2 = t + 0.5, i = floor(t2) (0 .. N), d = t2 - i - 0.5: cells (i - 1) mod N, i mod N, (i + 1) mod N get the same three weights
// and the particle adds m x the product of its per-axis weights to 2^dim / 3^dim cells.  No product is contracted into an FMA: the functions
// that evaluate weights carry `#pragma clang fp contract(off)` (the HIP headers' __dmul_rn is a plain product and contracts like one),
// so every weight is the fp64 number that the same expression gives on the host.
//
// Tile-owned form.  The particles are sorted by the tile of their BASE cell (CIC: i mod N; TSC: i; shifted: i mod N) with the NGP sort as it is: the key
// is dep_key of the base cell, and the 8-byte payload column that carries the masses for NGP carries the particle's INDEX (as a double,
// exact below 2^53).  A workgroup per tile gathers x, y, z, m by that index, evaluates the weights again and accumulates in an LDS box of
// the tile plus its halo (CIC: one cell on the upper side of every axis, 17 x 17 x 33 doubles = 76 KB; TSC: one cell on both sides,
// 18 x 18 x 34 = 88 KB; 2-D: 65 x 129 = 67 KB and 66 x 130 = 69 KB: dynamic LDS, one workgroup per CU).  The tile's own cells are stored once
// with plain stores (no zero-fill of the map); the halo cells -- and, on a partial tile, the cells of the box that lie past the grid's
// last cell, where the wrap lands -- go to the tile's slab of a halo scratch, and deposit_cloud_fold_kernel adds every non-zero entry of
// the scratch to the (wrapped) cell of the map with a global fp64 atomic in a second launch.  A tile that is its own neighbour through
// the wrap needs nothing special: its halo entries are added to its own stored cells like anyone else's.
//
//   deposit_cloud_keys_kernel    x, y, z -> key of the base cell, index payload, level-1 histograms (the role of deposit_keys_kernel)
//   deposit_cloud_tiles_kernel   workgroup per tile: gather, LDS accumulate (ds_add_f64), store own cells and the halo slab
//   deposit_cloud_fold_kernel    workgroup per tile: halo slab -> global atomics
//   deposit_cloud_atomic_kernel  one thread per particle, global atomics into a zero-filled map
#pragma once
#include "bfgx_deposit.hpp"

namespace bfgx {

// one axis of one particle.  c: the base cell the particle is sorted by (CIC: i mod N; TSC: i; SHIFT: i mod N); the cloud's cells are
// c - LO + k (mod N), k = 0 .. ORDER - 1, with LO = 0 (CIC) or 1 (TSC), and w[k] their weights.  false: the particle is dropped.
template <int ORDER, bool SHIFT = false>
__device__ inline bool cloud_axis(double v, double L, double s, int N, int &c, double (&w)[ORDER])
{
#pragma clang fp contract(off)
    static_assert(ORDER == 2 || ORDER == 3, "CIC or TSC");
    if (!(v >= 0.0) || !(v <= L)) return false;
    const double t = v * s;
    if constexpr (SHIFT && ORDER == 2) {
        const double fl = floor(t), f = t - fl;
        const int i = (int)fl;                               // 0 .. N
        w[0] = 1.0 - f; w[1] = f;
        c = (i >= N) ? 0 : i;
    } else if constexpr (SHIFT) {
        const double t2 = t + 0.5, fl = floor(t2);
        const int i = (int)fl;                               // 0 .. N
        const double d = t2 - fl - 0.5, a = 0.5 - d, b = 0.5 + d;
        w[0] = 0.5 * (a * a); w[1] = 0.75 - d * d; w[2] = 0.5 * (b * b);
        c = (i >= N) ? 0 : i;
    } else if constexpr (ORDER == 2) {
        const double u = t - 0.5, fl = floor(u), f = u - fl;
        const int i = (int)fl;                               // -1 .. N - 1
        w[0] = 1.0 - f; w[1] = f;
        c = (i < 0) ? N - 1 : min(i, N - 1);
    } else {
        const int i = min((int)floor(t), N - 1);
        const double d = t - (double)i - 0.5, a = 0.5 - d, b = 0.5 + d;
        w[0] = 0.5 * (a * a); w[1] = 0.75 - d * d; w[2] = 0.5 * (b * b);
        c = i;
    }
    return true;
}

template <int ORDER> struct CloudBox {
    static constexpr int H = ORDER - 1;              // halo cells per axis
    static constexpr int LO = (ORDER == 3) ? 1 : 0;  // of which below the tile
};

// doubles of the LDS box / of one tile's halo slab (the box less the tile)
__host__ __device__ inline int cloud_box_cells(const DepGeom &g, int order)
{
    const int h = order - 1;
    return (g.sx + h) * (g.sy + h) * (g.dim == 3 ? g.sz + h : 1);
}
__host__ __device__ inline int cloud_halo_cells(const DepGeom &g, int order) { return cloud_box_cells(g, order) - g.sx * g.sy * g.sz; }

// The halo cells of a tile whose own cells are ex x ey x ez (the tile shape clipped to the grid), numbered 0 .. count - 1: first the
// planes of the box outside the own range in x, then (x inside) those outside in y, then (x, y inside) those outside in z.  Box
// coordinate b of an axis is grid cell (tile origin) - LO + b; the own cells are LO <= b < LO + e.
template <int DIM, int ORDER> struct CloudHalo {
    static constexpr int H = CloudBox<ORDER>::H, LO = CloudBox<ORDER>::LO;
    int ex, ey, ez, eby, ebz, nX, nY, count;
    __device__ CloudHalo(const DepGeom &g, int x0, int y0, int z0)
    {
        ex = min(g.sx, g.nb - x0); ey = min(g.sy, g.nb - y0); ez = (DIM == 3) ? min(g.sz, g.nb - z0) : 1;
        eby = ey + H; ebz = (DIM == 3) ? ez + H : 1;
        nX = H * eby * ebz; nY = ex * H * ebz;
        count = nX + nY + ((DIM == 3) ? ex * ey * H : 0);
    }
    // the h-th halo coordinate of an axis with e own cells: below the tile first, then above
    __device__ static int outside(int h, int e) { return h < LO ? h : e + h; }
    __device__ void cell(int j, int &bx, int &by, int &bz) const
    {
        if (j < nX) {
            const int hx = j / (eby * ebz), r = j - hx * (eby * ebz);
            bx = outside(hx, ex); by = r / ebz; bz = r - by * ebz;
        } else if (j < nX + nY) {
            j -= nX;
            const int ix = j / (H * ebz), r = j - ix * (H * ebz), hy = r / ebz;
            bx = LO + ix; by = outside(hy, ey); bz = r - hy * ebz;
        } else {
            j -= nX + nY;
            const int ix = j / (ey * H), r = j - ix * (ey * H), iy = r / H;
            bx = LO + ix; by = LO + iy; bz = outside(r - iy * H, ez);
        }
    }
};

// grid cell of (tile origin) - LO + b, wrapped: the argument lies in [-1, N]
__device__ inline int cloud_wrap(int gx, int N) { return gx < 0 ? gx + N : (gx >= N ? gx - N : gx); }

template <int DIM, int ORDER, bool SHIFT = false>
__global__ void __launch_bounds__(256)
deposit_cloud_keys_kernel(DepGeom g, int64_t n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                          double L, double s, uint32_t *__restrict__ keys, double *__restrict__ index, int32_t *__restrict__ wg_hist, int64_t stride)
{
    __shared__ int hist[1024];
    const int tid = threadIdx.x;
    for (int i = tid; i < g.B1; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kDepChunk;
#pragma unroll 4
    for (int q = 0; q < kDepPer; ++q) {
        const int64_t p = base + q * 256 + tid;
        const bool on = p < n;
        const double vx = on ? x[p * stride] : 0.0, vy = on ? y[p * stride] : 0.0, vz = (DIM == 3 && on) ? z[p * stride] : 0.0;
        int cx = 0, cy = 0, cz = 0;
        double w[ORDER];
        bool inside = on && cloud_axis<ORDER, SHIFT>(vx, L, s, g.nb, cx, w) && cloud_axis<ORDER, SHIFT>(vy, L, s, g.nb, cy, w);
        if (DIM == 3) inside = inside && cloud_axis<ORDER, SHIFT>(vz, L, s, g.nb, cz, w);
        const uint32_t key = inside ? dep_key(g, cx, cy, cz) : kDepNoKey;
        lds_hist_rank(hist, (int)((key >> kDepLocalBits) >> g.lB2), inside);            // (every lane calls)
        if (on) { keys[p] = key; index[p] = (double)p; }
    }
    __syncthreads();
    for (int i = tid; i < g.B1; i += 256) wg_hist[(int64_t)i * gridDim.x + blockIdx.x] = hist[i];
}

constexpr int kCloudTileThreads = 1024;            // one workgroup per CU (67 - 88 KB of LDS): make it large
constexpr int kCloudFoldThreads = 256;

template <int DIM, int ORDER, bool SHIFT = false>
__global__ void __launch_bounds__(kCloudTileThreads)
deposit_cloud_tiles_kernel(DepGeom g, double L, double s, const int32_t *__restrict__ start2, const double *__restrict__ index,
                           const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                           const double *__restrict__ mass, int64_t stride, double *__restrict__ out, double *__restrict__ halo)
{
#pragma clang fp contract(off)
    constexpr int NT = kCloudTileThreads, H = CloudBox<ORDER>::H, LO = CloudBox<ORDER>::LO, LOZ = (DIM == 3) ? LO : 0;
    extern __shared__ double cloud_acc[];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const int BY = g.sy + H, BZ = (DIM == 3) ? g.sz + H : 1, ncell = (g.sx + H) * BY * BZ;
    for (int i = tid; i < ncell; i += NT) cloud_acc[i] = 0.0;
    __syncthreads();
    const int tz = tile % g.ntz, ty = (tile / g.ntz) % g.nty, tx = tile / (g.ntz * g.nty);
    const int x0 = tx * g.sx, y0 = ty * g.sy, z0 = tz * g.sz;
    const int s0 = start2[tile], s1 = start2[tile + 1];
    for (int i = s0 + tid; i < s1; i += NT) {
        const int64_t p = (int64_t)index[i];
        const double m = mass ? mass[p * stride] : 1.0;
        int cx = 0, cy = 0, cz = 0;
        double wx[ORDER], wy[ORDER], wz[ORDER];
        bool ok = cloud_axis<ORDER, SHIFT>(x[p * stride], L, s, g.nb, cx, wx) && cloud_axis<ORDER, SHIFT>(y[p * stride], L, s, g.nb, cy, wy);
        if (DIM == 3) ok = ok && cloud_axis<ORDER, SHIFT>(z[p * stride], L, s, g.nb, cz, wz);
        const int bx = cx - x0, by = cy - y0, bz = (DIM == 3) ? cz - z0 : 0;
        // (the sort brought the particle here because its base cell is in this tile; a box index is never taken on trust)
        if (!ok || bx < 0 || bx >= g.sx || by < 0 || by >= g.sy || bz < 0 || bz >= g.sz) continue;
#pragma unroll
        for (int a = 0; a < ORDER; ++a)
#pragma unroll
            for (int b = 0; b < ORDER; ++b) {
                const double wab = wx[a] * wy[b];
                double *row = cloud_acc + ((bx + a) * BY + (by + b)) * BZ + bz;
                if constexpr (DIM == 3) {
#pragma unroll
                    for (int c = 0; c < ORDER; ++c) atomicAdd(row + c, wab * wz[c] * m);
                } else atomicAdd(row, wab * m);
            }
    }
    __syncthreads();
    // the tile's own cells, stored once
    for (int l = tid; l < g.sx * g.sy * g.sz; l += NT) {
        const int lz = l & (g.sz - 1), ly = (l >> g.lsz) & (g.sy - 1), lx = l >> (g.lsz + g.lsy);
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        if (gx >= g.nb || gy >= g.nb || (DIM == 3 && gz >= g.nb)) continue;
        const int64_t flat = (DIM == 3) ? ((int64_t)gx * g.nb + gy) * g.nb + gz : (int64_t)gx * g.nb + gy;
        out[flat] = cloud_acc[((lx + LO) * BY + (ly + LO)) * BZ + lz + LOZ];
    }
    // the halo slab (deposit_cloud_fold_kernel skips the slab of a tile without particles, as this kernel does)
    if (s1 > s0) {
        const CloudHalo<DIM, ORDER> hc(g, x0, y0, z0);
        double *slab = halo + (int64_t)tile * cloud_halo_cells(g, ORDER);
        for (int j = tid; j < hc.count; j += NT) {
            int bx, by, bz;
            hc.cell(j, bx, by, bz);
            slab[j] = cloud_acc[(bx * BY + by) * BZ + bz];
        }
    }
}

template <int DIM, int ORDER>
__global__ void __launch_bounds__(kCloudFoldThreads)
deposit_cloud_fold_kernel(DepGeom g, const int32_t *__restrict__ start2, const double *__restrict__ halo, double *__restrict__ out)
{
    constexpr int LO = CloudBox<ORDER>::LO, LOZ = (DIM == 3) ? LO : 0;
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (start2[tile + 1] <= start2[tile]) return;
    const int tz = tile % g.ntz, ty = (tile / g.ntz) % g.nty, tx = tile / (g.ntz * g.nty);
    const int x0 = tx * g.sx, y0 = ty * g.sy, z0 = tz * g.sz;
    const CloudHalo<DIM, ORDER> hc(g, x0, y0, z0);
    const double *slab = halo + (int64_t)tile * cloud_halo_cells(g, ORDER);
    for (int j = tid; j < hc.count; j += kCloudFoldThreads) {
        const double v = slab[j];
        if (v == 0.0) continue;                                  // (most of a slab; NaN is added)
        int bx, by, bz;
        hc.cell(j, bx, by, bz);
        const int gx = cloud_wrap(x0 - LO + bx, g.nb), gy = cloud_wrap(y0 - LO + by, g.nb), gz = (DIM == 3) ? cloud_wrap(z0 - LOZ + bz, g.nb) : 0;
        const int64_t flat = (DIM == 3) ? ((int64_t)gx * g.nb + gy) * g.nb + gz : (int64_t)gx * g.nb + gy;
        atomicAdd(out + flat, v);
    }
}

// one thread per particle, 2^dim / 3^dim global atomics into a zero-filled map
template <int DIM, int ORDER, bool SHIFT = false>
__global__ void __launch_bounds__(256)
deposit_cloud_atomic_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                            const double *__restrict__ mass, int nb, double L, double s, double *__restrict__ out, int64_t stride)
{
#pragma clang fp contract(off)
    constexpr int LO = CloudBox<ORDER>::LO;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int cx = 0, cy = 0, cz = 0;
    double wx[ORDER], wy[ORDER], wz[ORDER];
    bool ok = cloud_axis<ORDER, SHIFT>(x[p * stride], L, s, nb, cx, wx) && cloud_axis<ORDER, SHIFT>(y[p * stride], L, s, nb, cy, wy);
    if (DIM == 3) ok = ok && cloud_axis<ORDER, SHIFT>(z[p * stride], L, s, nb, cz, wz);
    if (!ok) return;
    const double m = mass ? mass[p * stride] : 1.0;
#pragma unroll
    for (int a = 0; a < ORDER; ++a) {
        const int gx = cloud_wrap(cx - LO + a, nb);
#pragma unroll
        for (int b = 0; b < ORDER; ++b) {
            const int gy = cloud_wrap(cy - LO + b, nb);
            const double wab = wx[a] * wy[b];
            if constexpr (DIM == 3) {
#pragma unroll
                for (int c = 0; c < ORDER; ++c)
                    atomicAdd(out + ((int64_t)gx * nb + gy) * nb + cloud_wrap(cz - LO + c, nb), wab * wz[c] * m);
            } else atomicAdd(out + (int64_t)gx * nb + gy, wab * m);
        }
    }
}

}  // namespace bfgx
