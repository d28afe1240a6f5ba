// cluster_uf.h -- the union-find and the adjacency of the friends-of-friends clusters (cluster_kernels.hip), written
// so that a host program can compile the same text: the device takes the integer atomicMin, a host build (serial) a
// plain minimum.  The estimator is written down at c21cm_bubble_clusters_grids (include/c21cm_grid.h).
//
// The forest: label[i] <= i at all times and a label only ever decreases, so every find descends strictly and ends,
// whatever other threads do meanwhile; the root of a tree is its smallest cell.  No thread waits for another.
#ifndef C21_CLUSTER_UF_H
#define C21_CLUSTER_UF_H

#if defined(__HIPCC__)
#define C21_UF_FN __host__ __device__ __forceinline__
#else
#define C21_UF_FN static inline
#endif

// the label of cell c as other threads may be writing it
C21_UF_FN int c21_uf_load(const int *label, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(label + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return label[c];
#endif
}

// min(label[c], v) stored, the value before returned
C21_UF_FN int c21_uf_min(int *label, int c, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(label + c, v);
#else
    const int old = label[c];
    if (v < old) label[c] = v;
    return old;
#endif
}

// the root above c: every step goes to a strictly smaller cell
C21_UF_FN int c21_uf_find(const int *label, int c) {
    for (;;) {
        const int up = c21_uf_load(label, c);
        if (up >= c || up < 0) return c;  // up == c: a root (neither up > c nor the -1 of a cell that is not
                                          // selected can be met; both end the walk all the same)
        c = up;
    }
}

// find that shortens the path it walks (path halving): every other cell on the way is hung below its grandparent, by
// atomicMin, so a label still only decreases and still names a cell above it in the same tree.  The unions of a
// cluster that spans the box would otherwise walk chains of thousands of rows.
C21_UF_FN int c21_uf_find_halving(int *label, int c) {
    for (;;) {
        const int up = c21_uf_load(label, c);
        if (up >= c || up < 0) return c;
        const int top = c21_uf_load(label, up);
        if (top >= up || top < 0) return up;
        c21_uf_min(label, c, top);  // top < up < c
        c = top;
    }
}

// Joins the trees of a and b.  The larger root is hung below the smaller with one atomicMin; where another thread
// hung it first, the value it left (strictly below the root, or the loop would have ended) is what is joined with
// the smaller root next: the link the minimum may have replaced is made again one level further down.
C21_UF_FN void c21_uf_union(int *label, int a, int b) {
    for (;;) {
        a = c21_uf_find_halving(label, a);
        b = c21_uf_find_halving(label, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = c21_uf_min(label, a, b);  // b < a
        if (old == a) return;
        a = old;  // old < a: re-read from a label that has strictly decreased
    }
}

// the coordinate i + d on an axis of n cells, -1 through an open face
C21_UF_FN int c21_cl_step(int i, int d, int n, int periodic) {
    const int v = i + d;
    if (v >= 0 && v < n) return v;
    if (!periodic) return -1;
    return v < 0 ? n - 1 : 0;  // n = 1: the cell itself; n = 2: both sides the same cell
}

C21_UF_FN int c21_cl_bit(const unsigned long long *mask, long long row, int W, int z) {
    return (int)((mask[row * W + (z >> 6)] >> (z & 63)) & 1ull);
}

// the first cell of the z-run that holds the selected cell z of a row: the highest clear bit below it, a word at a time
C21_UF_FN int c21_cl_run_first(const unsigned long long *mask, long long row, int W, int z) {
    int wi = z >> 6;
    unsigned long long clear = ~mask[row * W + wi] & ((1ull << (z & 63)) - 1ull);
    while (!clear) {
        if (--wi < 0) return 0;
        clear = ~mask[row * W + wi];  // a word before the last of a row has no padding bits
    }
    return wi * 64 + 64 - (int)__builtin_clzll(clear);
}

// Joins the run start (ix, iy, iz) of a box to its selected neighbours, the offsets taken as the estimator lists them.
// Run starts suffice: of two runs in different rows that touch, the one that starts later starts beside the other
// (or diagonally below its end), and a cell at z = 0 is always a start, which covers the z wrap.
// In a row whose three cells at iz - 1, iz, iz + 1 are all neighbours, the selected ones among them are one cluster
// already where the middle one is selected (cells next to each other in z, through the wrap too, are neighbours at
// every connectivity), so one union with the middle cell serves the three.
C21_UF_FN void c21_cl_join_start(int *label, const unsigned long long *mask, int nx, int ny, int nz, int W, int ix,
                                 int iy, int iz, int connectivity, int periodic_mask) {
    const int self = (ix * ny + iy) * nz + iz;
    const int below = c21_cl_step(iz, -1, nz, (periodic_mask >> 2) & 1);
    const int above = c21_cl_step(iz, 1, nz, (periodic_mask >> 2) & 1);
    for (int dx = -1; dx <= 1; ++dx) {
        const int jx = c21_cl_step(ix, dx, nx, periodic_mask & 1);
        if (jx < 0) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int jy = c21_cl_step(iy, dy, ny, (periodic_mask >> 1) & 1);
            if (jy < 0) continue;
            const int n_set = (dx != 0) + (dy != 0);
            if (n_set > connectivity) continue;
            const long long row = (long long)jx * ny + jy;
            if (n_set && c21_cl_bit(mask, row, W, iz)) {  // offset (dx, dy, 0)
                c21_uf_union(label, self, (int)(row * nz + iz));
                continue;
            }
            if (n_set + 1 > connectivity) continue;
            if (below >= 0 && c21_cl_bit(mask, row, W, below)) c21_uf_union(label, self, (int)(row * nz + below));
            if (above >= 0 && c21_cl_bit(mask, row, W, above)) c21_uf_union(label, self, (int)(row * nz + above));
        }
    }
}

#endif
