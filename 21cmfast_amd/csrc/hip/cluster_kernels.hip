// cluster_kernels.hip -- friends-of-friends clusters of the selected cells of boxes and lightcone chunks (DESIGN
// 4.11; the estimator is written down at c21cm_bubble_clusters_grids, its spec is tests/cluster_reference.py).  The
// input is the bit mask of bubble_kernels.hip's pack; every launch covers all boxes (blockIdx.y = box).
//   init     a wave per mask word, a lane per cell: the label of a selected cell is the first cell of its z-run (the
//            highest clear bit below it, a word at a time), -1 elsewhere; the cell's size counter is zeroed.  This
//            settles every +-z adjacency inside a row without a union.  Lanes past nz store nothing.
//   merge    the run starts join their selected neighbours (cluster_uf.h: why run starts suffice): lock-free unions
//            on the global labels, the neighbour tests read from the mask.  This one pass also covers the periodic
//            faces and the z wrap.  A wave compacts the run starts of 32 mask words onto its lanes, and the finds
//            halve the paths they walk;
//   count    flatten and count in one pass: label[c] = find(c), size[root] += 1, pre-reduced: the lanes of a wave
//            that hold the same root add once (a ballot against the first remaining lane's root), a wave carries the
//            root it met last from word to word, and a workgroup sums what its waves let go of in an LDS table keyed
//            by the root before the integer atomics;
//   roots    the cells with label[c] == c, packed into a second bit mask with its chunk counts, so that
//            c21hip_bubble_rank gives the number of clusters and every root's rank;
//   emit     one lane per root: (root, size) at its rank where asked for, the size binned through LDS counters
//            flushed with 64-bit integer atomics, the largest cluster by one atomicMax on (size << 32) | (2^31 - 1 -
//            root), which resolves ties to the smallest root;
//   finish   the four stats of every box.
// Only integer atomics: two calls give the same bytes, and no result depends on the launch shape.  The forest keeps
// label[i] <= i and labels only decrease; no thread waits for another (cluster_uf.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"
#include "cluster_uf.h"
#include "wave_bits.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = C21HIP_BUBBLE_CHUNK;
constexpr int kMergeWords = 32;     // mask words (2048 cells) whose run starts a merge wave hands to its lanes
constexpr int kCountBlocks = 4096;  // workgroups per box of the count pass at the most (16 per CU)
constexpr int kCountSlots = 1024;   // (root, cells) entries of a count workgroup's LDS table: 8 KiB
constexpr int kEmitBlocks = 2048;  // workgroups per box of the emit pass at the most (8 per CU)
static_assert(kChunk % kWaves == 0, "the root pack's waves share a chunk evenly");
static_assert(kCountSlots == 1 << 10, "count_add hashes a root to 10 bits");

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

struct box_geom {
    int nx, ny, nz, W;
    long long words, cells;  // per box
};

// wave (blockIdx.x kWaves + wave) owns word g of box b; false past the last word
__device__ __forceinline__ bool word_of_wave(const box_geom &s, long long *g, long long *row, int *z) {
    *g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (*g >= s.words) return false;
    *row = *g / s.W;
    *z = (int)(*g - *row * s.W) * 64 + (int)(threadIdx.x & 63);
    return true;
}

__global__ __launch_bounds__(kBlock) void cluster_init_kernel(box_geom s, const unsigned long long *__restrict__ mask,
                                                              int *__restrict__ label, int *__restrict__ size) {
    long long g, row;
    int z;
    if (!word_of_wave(s, &g, &row, &z) || z >= s.nz) return;
    const unsigned long long *m = mask + (long long)blockIdx.y * s.words;
    const long long c = (long long)blockIdx.y * s.cells + row * s.nz + z;
    label[c] = c21_cl_bit(m, row, s.W, z) ? (int)(row * s.nz) + c21_cl_run_first(m, row, s.W, z) : -1;
    size[c] = 0;
}

// A wave owns kMergeWords consecutive mask words and gives its lanes the run starts among their cells, 64 at a
// time: a union is a chain of dependent loads, so the lanes that wait on one should all have one to wait on (a smooth
// field has one or two starts per 64 cells).
// Lane q holds the start bits of word q (word & ~(word << 1), the carry from the word before in the row); a scan of
// their counts numbers the starts, and start i is found by a search over the lanes' counts and a select in the word.
__global__ __launch_bounds__(kBlock) void cluster_merge_kernel(box_geom s, const unsigned long long *__restrict__ mask,
                                                               int *label, int connectivity, int periodic_mask) {
    const int lane = threadIdx.x & 63;
    const long long g0 = ((long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * kMergeWords;
    if (g0 >= s.words) return;  // the whole wave
    const unsigned long long *m = mask + (long long)blockIdx.y * s.words;
    int *l = label + (long long)blockIdx.y * s.cells;
    unsigned long long starts = 0ull;
    if (lane < kMergeWords && g0 + lane < s.words) {
        const long long g = g0 + lane;
        const unsigned long long word = m[g];
        const unsigned long long before = g % s.W ? m[g - 1] >> 63 : 0ull;
        starts = word & ~((word << 1) | before);
    }
    const int mine = __popcll(starts);
    const int incl = wave_inclusive(mine, lane);
    const int total = __shfl(incl, 63, 64);
    for (int base = 0; base < total; base += 64) {  // uniform over the wave
        const bool active = base + lane < total;
        const int i = active ? base + lane : total - 1;
        int lo = 0, hi = 63;  // the first lane whose inclusive count is above i
#pragma unroll
        for (int step = 0; step < 6; ++step) {
            const int mid = (lo + hi) >> 1;
            if (__shfl(incl, mid, 64) > i) hi = mid;
            else lo = mid + 1;
        }
        const unsigned long long word = __shfl(starts, lo, 64);
        const int first = __shfl(incl - mine, lo, 64);
        if (!active) continue;
        const long long g = g0 + lo;
        const long long row = g / s.W;
        const int z = (int)(g - row * s.W) * 64 + select_bit(word, i - first);
        const int ix = (int)(row / s.ny);
        c21_cl_join_start(l, m, s.nx, s.ny, s.nz, s.W, ix, (int)(row - (long long)ix * s.ny), z, connectivity,
                          periodic_mask);
    }
}

// the (root, cells) pair of a wave goes into the workgroup's table where its slot or one of the next three is free
// or holds the root already, and straight to the global counter otherwise
__device__ __forceinline__ void count_add(int *key, int *num, int *sz, int root, int n) {
    const unsigned h = ((unsigned)root * 2654435761u) >> 22;
    for (unsigned probe = 0; probe < 4; ++probe) {
        const unsigned slot = (h + probe) & (kCountSlots - 1);
        const int old = atomicCAS(&key[slot], -1, root);
        if (old == -1 || old == root) {
            atomicAdd(&num[slot], n);
            return;
        }
    }
    atomicAdd(&sz[root], n);
}

// flatten and count in one pass over the cells: label[c] = find(c), size[root] += 1.  A wave runs through words a
// grid stride apart; per word the lanes that hold the same root add once, the wave carries the root it met last
// into the next word, and what it lets go of is summed per workgroup in an LDS table keyed by the root, flushed with
// one atomic per entry: near percolation the one hot root takes one atomic per workgroup, not one per wave and word
__global__ __launch_bounds__(kBlock) void cluster_count_kernel(box_geom s, int *label, int *__restrict__ size) {
    __shared__ int key[kCountSlots], num[kCountSlots];
    for (int i = threadIdx.x; i < kCountSlots; i += kBlock) {
        key[i] = -1;
        num[i] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int *l = label + (long long)blockIdx.y * s.cells;
    int *sz = size + (long long)blockIdx.y * s.cells;
    const long long stride = (long long)gridDim.x * kWaves;
    int held = -1, n_held = 0;
    for (long long g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); g < s.words; g += stride) {
        const long long row = g / s.W;
        const int z = (int)(g - row * s.W) * 64 + lane;
        int root = -1;
        if (z < s.nz) {
            const int c = (int)(row * s.nz + z);
            const int up = l[c];  // -1 where the cell is not selected
            if (up >= 0) {
                root = c21_uf_find(l, up);
                if (root != up) l[c] = root;
            }
        }
        unsigned long long left = __ballot(root >= 0);
        while (left) {  // uniform over the wave
            const int r0 = __shfl(root, __ffsll((long long)left) - 1, 64);
            const unsigned long long same = __ballot(root == r0);
            left &= ~same;
            if (r0 == held) {
                n_held += __popcll(same);
            } else {
                if (n_held && lane == 0) count_add(key, num, sz, held, n_held);
                held = r0;
                n_held = __popcll(same);
            }
        }
    }
    if (n_held && lane == 0) count_add(key, num, sz, held, n_held);
    __syncthreads();
    for (int i = threadIdx.x; i < kCountSlots; i += kBlock)
        if (key[i] >= 0) atomicAdd(&sz[key[i]], num[i]);
}

// workgroup (c, b): words [64 c, 64 c + 64) of box b, 16 per wave; bit = the cell is the root of its cluster
__global__ __launch_bounds__(kBlock) void cluster_roots_kernel(box_geom s, const int *__restrict__ label,
                                                               unsigned long long *__restrict__ root_mask,
                                                               int *__restrict__ chunk_sum, int n_chunks) {
    __shared__ int wave_sum[kWaves];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int *l = label + (long long)b * s.cells;
    constexpr int kPer = kChunk / kWaves;
    const long long g0 = (long long)blockIdx.x * kChunk + wave * kPer;
    int count = 0;
    unsigned long long mine = 0ull;
    for (int q = 0; q < kPer; ++q) {
        const long long g = g0 + q;
        bool is_root = false;
        if (g < s.words) {
            const long long row = g / s.W;
            const int z = (int)(g - row * s.W) * 64 + lane;
            if (z < s.nz) {
                const long long c = row * s.nz + z;
                is_root = l[c] == (int)c;
            }
        }
        const unsigned long long word = __ballot(is_root);
        if (lane == q) mine = word;
        count += __popcll(word);
    }
    if (lane < kPer && g0 + lane < s.words) root_mask[(long long)b * s.words + g0 + lane] = mine;
    if (lane == 0) wave_sum[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kWaves; ++w) t += wave_sum[w];
        chunk_sum[(long long)b * n_chunks + blockIdx.x] = t;
    }
}

// dynamic LDS: best key (64 bits) | cells per bin (64 bits) [n_bins] | clusters per bin (32 bits) [n_bins]
__global__ __launch_bounds__(kBlock) void cluster_emit_kernel(box_geom s, c21hip_cluster_emit_args a) {
    extern __shared__ unsigned long long lds[];
    const int nb = a.n_bins;
    unsigned long long *best = lds, *cells = lds + 1;
    unsigned int *cnt = (unsigned int *)(lds + 1 + nb);
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        cells[i] = 0ull;
        cnt[i] = 0u;
    }
    if (threadIdx.x == 0) *best = 0ull;
    __syncthreads();

    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const unsigned long long *rm = a.root_mask + (long long)b * s.words;
    const long long *prefix = a.prefix + (long long)b * s.words;
    const int *sz = a.size + (long long)b * s.cells;
    const long long stride = (long long)gridDim.x * kWaves;
    for (long long g = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); g < s.words; g += stride) {
        const unsigned long long word = rm[g];
        if (!((word >> lane) & 1ull)) continue;  // a padding bit is never set
        const long long row = g / s.W;
        const long long c = row * s.nz + (g - row * s.W) * 64 + lane;
        const long long rank = prefix[g] + __popcll(word & ((1ull << lane) - 1ull));
        const long long n = sz[c];
        if (a.roots && rank < a.max_clusters) {
            a.roots[(long long)b * a.max_clusters + rank] = c;
            a.sizes[(long long)b * a.max_clusters + rank] = n;
        }
        atomicMax(best, ((unsigned long long)n << 32) | (unsigned long long)(0x7FFFFFFFll - c));
        // np.digitize (increasing edges): the number of edges <= n, less one
        int lo = 0, hi = nb + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.edges[mid] <= n) lo = mid + 1;
            else hi = mid;
        }
        const int bin = lo - 1;
        if (bin >= 0 && bin < nb) {
            atomicAdd(&cnt[bin], 1u);
            atomicAdd(&cells[bin], (unsigned long long)n);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        const unsigned int k = cnt[i];
        if (!k) continue;
        atomicAdd(&a.hist_n[(long long)b * nb + i], (unsigned long long)k);
        atomicAdd(&a.hist_cells[(long long)b * nb + i], cells[i]);
    }
    if (threadIdx.x == 0 && *best) atomicMax(&a.best[b], *best);
}

// stats[b] = {n_selected (as c21hip_bubble_rank left it), n_clusters, the largest cluster's cells, its root}
__global__ void cluster_finish_kernel(int n_batch, const long long *__restrict__ n_clusters,
                                      const unsigned long long *__restrict__ best, long long *__restrict__ stats) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_batch) return;
    const unsigned long long key = best[b];
    stats[4 * (long long)b + 1] = n_clusters[4 * (long long)b];
    stats[4 * (long long)b + 2] = (long long)(key >> 32);
    stats[4 * (long long)b + 3] = key ? 0x7FFFFFFFll - (long long)(key & 0xFFFFFFFFull) : -1;
}

// false where the shape does not fit the launches
bool geom_of(int nx, int ny, int nz, int n_batch, box_geom *s) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || n_batch > 65535) return false;
    if ((long long)nx * ny > 0x7FFFFFFFll || (long long)nx * ny * nz > 0x7FFFFFFFll) return false;
    s->nx = nx, s->ny = ny, s->nz = nz, s->W = (nz + 63) / 64;
    s->words = (long long)nx * ny * s->W;
    s->cells = (long long)nx * ny * nz;
    return (s->words + kWaves - 1) / kWaves <= 0x7FFFFFFFll;
}
}  // namespace

extern "C" int c21hip_cluster_label(const unsigned long long *mask, int nx, int ny, int nz, int n_batch,
                                    int connectivity, int periodic_mask, int *label, int *size, void *stream) {
    box_geom s;
    if (!geom_of(nx, ny, nz, n_batch, &s) || connectivity < 1 || connectivity > 3 || periodic_mask < 0 ||
        periodic_mask > 7 || !mask || !label || !size) {
        c21hip_set_error("cluster label: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const dim3 per_word((unsigned)((s.words + kWaves - 1) / kWaves), (unsigned)n_batch);
    hipLaunchKernelGGL(cluster_init_kernel, per_word, dim3(kBlock), 0, (hipStream_t)stream, s, mask, label, size);
    int status = launch_status("cluster init");
    if (status) return status;
    const long long merge_waves = (s.words + kMergeWords - 1) / kMergeWords;
    hipLaunchKernelGGL(cluster_merge_kernel, dim3((unsigned)((merge_waves + kWaves - 1) / kWaves), (unsigned)n_batch),
                       dim3(kBlock), 0, (hipStream_t)stream, s, mask, label, connectivity, periodic_mask);
    if ((status = launch_status("cluster merge"))) return status;
    long long blocks = (s.words + kWaves - 1) / kWaves;
    if (blocks > kCountBlocks) blocks = kCountBlocks;
    hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)blocks, (unsigned)n_batch), dim3(kBlock), 0,
                       (hipStream_t)stream, s, label, size);
    return launch_status("cluster count");
}

extern "C" int c21hip_cluster_roots(const int *label, int nx, int ny, int nz, int n_batch,
                                    unsigned long long *root_mask, int *chunk_sum, void *stream) {
    box_geom s;
    if (!geom_of(nx, ny, nz, n_batch, &s) || !label || !root_mask || !chunk_sum) {
        c21hip_set_error("cluster roots: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long chunks = (s.words + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(cluster_roots_kernel, dim3((unsigned)chunks, (unsigned)n_batch), dim3(kBlock), 0,
                       (hipStream_t)stream, s, label, root_mask, chunk_sum, (int)chunks);
    return launch_status("cluster roots");
}

extern "C" int c21hip_cluster_emit(const c21hip_cluster_emit_args *a, void *stream) {
    box_geom s;
    if (!a || !geom_of(a->nx, a->ny, a->nz, a->n_batch, &s) || a->n_bins < 1 || a->n_bins > C21HIP_BUBBLE_MAX_BINS ||
        !a->root_mask || !a->prefix || !a->size || !a->edges || !a->hist_n || !a->hist_cells || !a->best ||
        !a->n_clusters || !a->stats || (a->roots != NULL) != (a->sizes != NULL) || (a->roots && a->max_clusters < 1)) {
        c21hip_set_error("cluster emit: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    long long blocks = (s.words + kWaves - 1) / kWaves;
    if (blocks > kEmitBlocks) blocks = kEmitBlocks;
    const size_t lds = sizeof(unsigned long long) * (1 + (size_t)a->n_bins) + sizeof(unsigned int) * (size_t)a->n_bins;
    hipLaunchKernelGGL(cluster_emit_kernel, dim3((unsigned)blocks, (unsigned)a->n_batch), dim3(kBlock), lds,
                       (hipStream_t)stream, s, *a);
    int status = launch_status("cluster emit");
    if (status) return status;
    hipLaunchKernelGGL(cluster_finish_kernel, dim3((unsigned)((a->n_batch + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, a->n_batch, a->n_clusters, a->best, a->stats);
    return launch_status("cluster finish");
}
