#pragma once
// ---- connected components of a class map and the removal of small regions (cvk_cc_label, cvk_cc_filter; the definitions are in
// include/cvk.h) --------------------------------------------------------------------------------------------------------------------
// A pixel's code is its class, or CC_VOID for every other value; a component is a maximal set of equal codes of one image connected
// under 4 or 8 neighbours; its label is the row-major index y W + x of its first pixel.  Union-find over tiles of CC_TH x CC_TW pixels,
// every tree linked larger index -> smaller index, so a root is the smallest index of its set and the label needs no second pass:
//   k_cc_tile     work-group = one tile, codes and tile-local parents in LDS.  A row of the tile is one wave: the start of a pixel's
//                 horizontal run comes from one ballot, the parents start there.  Then one union per pair of vertically overlapping runs
//                 (at the first column of the overlap) and, under 8, the diagonals where the pixel above has another code.  The local
//                 order is monotone in the image order, so the local root is the tile's first pixel of the component.  Writes each
//                 pixel's parent as an index into its image, its code byte, and zeroes its area slot.
//   k_cc_merge    one thread per pixel of a tile's bottom row (pairs with the row below: straight, and under 8 both diagonals) or right
//                 column (the column to the right likewise).  Every read of the parent array is an agent-scope atomic load, every write an
//                 atomicMin: private L2s may hand out stale parents, and a stale parent is an older, larger member of the same set.
//   k_cc_flatten  labels[p] = find(p) by plain loads (the launch boundary published the parents, nothing writes them here); one
//                 atomicAdd into the root's area slot per run of equal roots in a wave.
//   k_cc_area     area[p] = area[root] for the pixels that are no root.
//   k_cc_prep     (filter) code bytes, the record's slots 0..4 and, for the vote, the root's own thread zeroes its [C] vote slots.
//   k_cc_vote     (filter, mode neighbour) a pixel of a small class component adds one vote per neighbour of a class whose component
//                 is not small.
//   k_cc_apply    (filter) writes out and the record's slots 5..7.
// Termination.  cc_find_*: a parent is never above its child and equals it only at a root, so every step lowers the index: at most
// `index` steps (the tile's 2047 in LDS).  cc_union_*: an iteration finds two roots a > b and ends when they are equal or when the
// atomicMin on a's slot returns a (a was a root, now linked); otherwise it returns old < a and the pair becomes (old, b), both below
// a: the larger index of the pair falls every iteration, so at most `index` iterations.  When a was no longer a root the atomicMin may
// have replaced a -> old by a -> b; old and b are then united by the next iteration, so no equivalence is lost.  Nothing waits for
// another work-group: no flag, no spin, no grid barrier.  The vote and record loops are bounded by 8 neighbours and by C.
// Which unions are made.  Inside a tile: runs of a row are joined by construction; two vertically adjacent runs of one code overlap in
// columns [a, b], and the pixel at a is either the start of its own run or of the run above, which is the test below.  Across a seam a
// straight pair at column x is skipped only when the pair at x - 1 has the same code on both sides and lies in the same tile column
// (rows alike), so the skipped pair follows from that one and two unions made inside tiles; a diagonal pair is skipped when the
// straight neighbour on the far side has the code too.  Pairs at a tile corner are never skipped.
// LDS: k_cc_tile 2 KiB codes + 8 KiB parents; k_cc_prep / k_cc_apply 1 KiB of record counters.
#include "cvk_common.h"

namespace {

constexpr int CC_MAX_K = 32, CC_TH = 32, CC_TW = 64, CC_TILE = CC_TH * CC_TW;
constexpr int CC_RECORD_SLOTS = 8, CC_BLOCK_PIXELS = 1024;
constexpr unsigned char CC_VOID = 254, CC_OUTSIDE = 255;
enum { CC_COMPONENTS = 0, CC_PIXELS, CC_LARGEST, CC_SMALL, CC_SMALL_PIXELS, CC_CHANGED, CC_RECEIVED, CC_ISOLATED };

__device__ __forceinline__ unsigned char cc_code(int64_t v, int K, int ignore) {
    return (v >= 0 && v < K && v != (int64_t)ignore) ? (unsigned char)v : CC_VOID;
}

__device__ __forceinline__ int cc_find_lds(int* loc, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&loc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p >= i) return i;
        i = p;
    }
}

__device__ __forceinline__ void cc_union_lds(int* loc, int a, int b) {
    for (;;) {
        a = cc_find_lds(loc, a);
        b = cc_find_lds(loc, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&loc[a], b);
        if (old >= a) return;
        a = old;
    }
}

__device__ __forceinline__ int cc_find_agent(int* parent, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= i) return i;
        i = p;
    }
}

// parent: the image's own slice; a and b are indices into the image
__device__ __forceinline__ void cc_union_agent(int* parent, int a, int b) {
    for (;;) {
        a = cc_find_agent(parent, a);
        b = cc_find_agent(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&parent[a], b);
        if (old >= a) return;
        a = old;
    }
}

// grid N * tiles_y * tiles_x, 256 threads: wave w owns rows 8 w .. 8 w + 7 of the tile, a lane one column
__global__ __launch_bounds__(256) void k_cc_tile(const int64_t* __restrict__ map, int* __restrict__ parent, unsigned char* __restrict__ codes,
                                                int* __restrict__ area, int H, int W, int tiles_x, int tiles_y, int K, int ignore, int conn8) {
    __shared__ unsigned char s_code[CC_TILE];
    __shared__ int s_loc[CC_TILE];
    const int per = tiles_x * tiles_y, n = blockIdx.x / per, rem = blockIdx.x - n * per;
    const int y0 = (rem / tiles_x) * CC_TH, x0 = (rem % tiles_x) * CC_TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gx = x0 + lane;
    const size_t img = (size_t)n * H * W;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int y = wave * 8 + r, gy = y0 + y, i = y * CC_TW + lane;
        const bool in = gx < W && gy < H;
        unsigned char c = CC_OUTSIDE;
        if (in) {
            const size_t g = img + (size_t)gy * W + gx;
            c = cc_code(map[g], K, ignore);
            codes[g] = c;
            area[g] = 0;
        }
        const int left = __shfl_up((int)c, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || left != (int)c);   // bit 0 is always set
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        s_code[i] = c;
        s_loc[i] = y * CC_TW + start;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int y = wave * 8 + r, i = y * CC_TW + lane;
        const int c = s_code[i];
        if (y == 0 || c == CC_OUTSIDE) continue;
        const int up = s_code[i - CC_TW];
        const int l = lane > 0 ? s_code[i - 1] : -1, ul = lane > 0 ? s_code[i - CC_TW - 1] : -1;
        const int ur = lane < CC_TW - 1 ? s_code[i - CC_TW + 1] : -1;
        if (up == c) {
            if (l != c || ul != c) cc_union_lds(s_loc, i, i - CC_TW);
        } else if (conn8) {
            if (ul == c) cc_union_lds(s_loc, i, i - CC_TW - 1);
            if (ur == c) cc_union_lds(s_loc, i, i - CC_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int y = wave * 8 + r, gy = y0 + y, i = y * CC_TW + lane;
        if (gx < W && gy < H) {
            const int root = cc_find_lds(s_loc, i);
            parent[img + (size_t)gy * W + gx] = (y0 + root / CC_TW) * W + x0 + root % CC_TW;
        }
    }
}

// threads [0, total_h): pixel (x, y) on the bottom row of a tile row that has a row below it; [total_h, total_h + total_v): pixel on
// the right column of a tile column that has a column to its right
__global__ __launch_bounds__(256) void k_cc_merge(int* parent, const unsigned char* __restrict__ codes, int H, int W, int seams_y,
                                                 int seams_x, int total_h, int total_v, int conn8) {
    const int t = blockIdx.x * 256 + threadIdx.x;        // the grid covers total_h + total_v < 2^31 with less than 256 to spare
    if (t >= total_h + total_v) return;
    const int HW = H * W;
    if (t < total_h) {
        const int per = seams_y * W, n = t / per, rem = t - n * per, j = rem / W, x = rem - j * W, y = j * CC_TH + CC_TH - 1;
        const unsigned char* cd = codes + (size_t)n * HW;
        int* par = parent + (size_t)n * HW;
        const int a = y * W + x, c = cd[a], dn = cd[a + W];
        if (dn == c) {
            if (x % CC_TW == 0 || cd[a - 1] != c || cd[a + W - 1] != c) cc_union_agent(par, a, a + W);
        } else if (conn8) {
            if (x > 0 && cd[a + W - 1] == c) cc_union_agent(par, a, a + W - 1);
            if (x + 1 < W && cd[a + W + 1] == c) cc_union_agent(par, a, a + W + 1);
        }
    } else {
        const int u = t - total_h, per = seams_x * H, n = u / per, rem = u - n * per, j = rem / H, y = rem - j * H, x = j * CC_TW + CC_TW - 1;
        const unsigned char* cd = codes + (size_t)n * HW;
        int* par = parent + (size_t)n * HW;
        const int a = y * W + x, c = cd[a], rt = cd[a + 1];
        if (rt == c) {
            if (y % CC_TH == 0 || cd[a - W] != c || cd[a - W + 1] != c) cc_union_agent(par, a, a + 1);
        } else if (conn8) {
            if (y > 0 && cd[a - W + 1] == c) cc_union_agent(par, a, a - W + 1);
            if (y + 1 < H && cd[a + W + 1] == c) cc_union_agent(par, a, a + W + 1);
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_flatten(const int* __restrict__ parent, int* __restrict__ labels, int* __restrict__ area, int M,
                                                   int HW) {
    const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int groot = -1;                                        // the root as an index into the batch; -1 past the end
    if (p < M) {
        const int base = (p / HW) * HW;
        int r = p - base;
        for (;;) {
            const int pr = parent[base + r];
            if (pr >= r) break;
            r = pr;
        }
        labels[p] = r;
        groot = base + r;
    }
    const int prev = __shfl_up(groot, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != groot);
    if (groot >= 0 && (lane == 0 || prev != groot)) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = above ? __ffsll((long long)above) : 64 - lane;
        atomicAdd(&area[groot], len);
    }
}

__global__ __launch_bounds__(256) void k_cc_area(const int* __restrict__ labels, int* __restrict__ area, int M, int HW) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    const int root = (p / HW) * HW + labels[p];
    if (root != p) area[p] = area[root];
}

__device__ __forceinline__ void cc_record_flush(const unsigned* s_rec, unsigned long long* record, int n, int K) {
    for (int i = threadIdx.x; i < K * CC_RECORD_SLOTS; i += 256) {
        const unsigned v = s_rec[i];
        if (!v) continue;
        unsigned long long* dst = record + (size_t)n * K * CC_RECORD_SLOTS + i;
        if (i % CC_RECORD_SLOTS == CC_LARGEST) atomicMax(dst, (unsigned long long)v);
        else atomicAdd(dst, (unsigned long long)v);
    }
}

// Every lane of the wave calls it; lanes hold neighbouring pixels.  s_rec[key] += 1 per lane with key >= 0, as one LDS atomic per run of
// equal keys: neighbouring pixels mostly share their class, and 64 lanes on one LDS word would take turns.
__device__ __forceinline__ void cc_wave_count(unsigned* s_rec, int key) {
    const int lane = threadIdx.x & 63, prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (head && key >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        atomicAdd(&s_rec[key], (unsigned)(above ? __ffsll((long long)above) : 64 - lane));
    }
}

// grid N * blocks_per_image, 256 threads, CC_BLOCK_PIXELS pixels of one image per work-group.  votes: nullable (mode fill).
__global__ __launch_bounds__(256) void k_cc_prep(const int64_t* __restrict__ map, const int* __restrict__ labels, const int* __restrict__ area,
                                                unsigned char* __restrict__ codes, int* __restrict__ votes,
                                                unsigned long long* __restrict__ record, int HW, int K, int ignore, int min_area,
                                                int per_image) {
    __shared__ unsigned s_rec[CC_MAX_K * CC_RECORD_SLOTS];
    const int n = blockIdx.x / per_image, blk = blockIdx.x - n * per_image;
    const size_t img = (size_t)n * HW;
    if (record) {
        for (int i = threadIdx.x; i < K * CC_RECORD_SLOTS; i += 256) s_rec[i] = 0u;
        __syncthreads();
    }
    constexpr int IT = CC_BLOCK_PIXELS / 256;
    int64_t vs[IT];
    int as[IT], ls[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {                      // every load of the work-group's pixels first: they do not depend on each other
        const int q = blk * CC_BLOCK_PIXELS + it * 256 + threadIdx.x;
        const size_t g = img + (q < HW ? q : 0);
        vs[it] = map[g];
        as[it] = area[g];
        ls[it] = labels[g];
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {                      // no lane leaves the loop early: cc_wave_count needs the whole wave
        const int q = blk * CC_BLOCK_PIXELS + it * 256 + threadIdx.x;
        const size_t g = img + q;
        int c = CC_OUTSIDE, a = 0;
        bool small = false, root = false;
        if (q < HW) {
            c = cc_code(vs[it], K, ignore);
            codes[g] = (unsigned char)c;
            if (c < CC_MAX_K) {
                a = as[it];
                small = a < min_area;
                root = ls[it] == q;
                if (root && small && votes)
                    for (int k = 0; k < K; ++k) votes[g * K + k] = 0;
            }
        }
        if (record) {
            const bool cls = c < CC_MAX_K;
            cc_wave_count(s_rec, cls ? c * CC_RECORD_SLOTS + CC_PIXELS : -1);
            cc_wave_count(s_rec, cls && small ? c * CC_RECORD_SLOTS + CC_SMALL_PIXELS : -1);
            if (root) {
                unsigned* r = s_rec + c * CC_RECORD_SLOTS;
                atomicAdd(&r[CC_COMPONENTS], 1u);
                atomicMax(&r[CC_LARGEST], (unsigned)a);
                if (small) atomicAdd(&r[CC_SMALL], 1u);
            }
        }
    }
    if (record) {
        __syncthreads();
        cc_record_flush(s_rec, record, n, K);
    }
}

__global__ __launch_bounds__(256) void k_cc_vote(const unsigned char* __restrict__ codes, const int* __restrict__ labels,
                                                const int* __restrict__ area, int* __restrict__ votes, int M, int H, int W, int K,
                                                int min_area, int conn8) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    if (codes[p] >= CC_MAX_K || area[p] >= min_area) return;
    const int HW = H * W, base = (p / HW) * HW, q = p - base, y = q / W, x = q - y * W;
    int* slot = votes + (size_t)(base + labels[p]) * K;
    int kk[8];                                             // the voting neighbours' classes, -1: no vote
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        kk[j] = -1;
        const int dy = j < 4 ? (j == 0 ? -1 : j == 3 ? 1 : 0) : (j < 6 ? -1 : 1);      // 0..3: up, left, right, down; 4..7: the diagonals
        const int dx = j < 4 ? (j == 1 ? -1 : j == 2 ? 1 : 0) : ((j & 1) ? 1 : -1);
        if (j >= 4 && !conn8) continue;
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const int g = base + yy * W + xx, k = codes[g];
        if (k < CC_MAX_K && area[g] >= min_area) kk[j] = k;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {                          // one atomic per distinct class
        if (kk[j] < 0) continue;
        int cnt = 1;
#pragma unroll
        for (int i = j + 1; i < 8; ++i)
            if (kk[i] == kk[j]) {
                ++cnt;
                kk[i] = -1;
            }
        atomicAdd(&slot[kk[j]], cnt);
    }
}

// mode 0: fill, 1: neighbour.  fill_code: the code of fill_value.
__global__ __launch_bounds__(256) void k_cc_apply(const int64_t* __restrict__ map, const int* __restrict__ labels, const int* __restrict__ area,
                                                 const int* __restrict__ votes, int64_t* __restrict__ out,
                                                 unsigned long long* __restrict__ record, int HW, int K, int ignore, int min_area, int mode,
                                                 int64_t fill_value, int fill_code, int per_image) {
    __shared__ unsigned s_rec[CC_MAX_K * CC_RECORD_SLOTS];
    const int n = blockIdx.x / per_image, blk = blockIdx.x - n * per_image;
    const size_t img = (size_t)n * HW;
    if (record) {
        for (int i = threadIdx.x; i < K * CC_RECORD_SLOTS; i += 256) s_rec[i] = 0u;
        __syncthreads();
    }
    constexpr int IT = CC_BLOCK_PIXELS / 256;
    int64_t vs[IT];
    int as[IT], ls[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {                      // every load of the work-group's pixels first: they do not depend on each other
        const int q = blk * CC_BLOCK_PIXELS + it * 256 + threadIdx.x;
        const size_t g = img + (q < HW ? q : 0);
        vs[it] = map[g];
        as[it] = area[g];
        ls[it] = labels[g];
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {                      // no lane leaves the loop early: cc_wave_count needs the whole wave
        const int q = blk * CC_BLOCK_PIXELS + it * 256 + threadIdx.x;
        const bool in = q < HW;
        const size_t g = img + (in ? q : 0);
        const int64_t v = vs[it];
        int64_t o = v;
        const int c = cc_code(v, K, ignore);
        int received = -1;
        if (in && c < CC_MAX_K && as[it] < min_area) {
            const bool root = ls[it] == q;
            int to = -1;                                   // the class the pixel goes to, CC_VOID for a fill value that is no class
            if (mode == 0) {
                if (fill_value != v) {
                    o = fill_value;
                    to = fill_code;
                }
            } else {
                const int* slot = votes + (img + ls[it]) * K;
                int best = 0;
                for (int k = 0; k < K; ++k) {
                    const int s = slot[k];
                    if (s > best) {
                        best = s;
                        to = k;
                    }
                }
                if (to >= 0) o = to;
            }
            if (to >= 0 && to < CC_MAX_K) received = to * CC_RECORD_SLOTS + CC_RECEIVED;
            if (record) {
                if (root && to >= 0) atomicAdd(&s_rec[c * CC_RECORD_SLOTS + CC_CHANGED], 1u);
                if (root && to < 0 && mode == 1) atomicAdd(&s_rec[c * CC_RECORD_SLOTS + CC_ISOLATED], 1u);
            }
        }
        if (record) cc_wave_count(s_rec, received);
        if (in) out[g] = o;
    }
    if (record) {
        __syncthreads();
        cc_record_flush(s_rec, record, n, K);
    }
}

inline int64_t cc_round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline bool cc_sizes_ok(int N, int H, int W, int K) {
    return K >= 1 && K <= CC_MAX_K && N > 0 && H > 0 && W > 0 && (int64_t)N * H * W < 2147483648LL;
}

inline int cc_check(const char* who, int N, int H, int W, int K, int connectivity) {
    CVK_CHECK_ARG(K >= 1 && K <= CC_MAX_K, "%s: %d classes, the kernels serve 1 to %d", who, K, CC_MAX_K);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: sizes must be positive, got N %d, H %d, W %d", who, N, H, W);
    CVK_CHECK_ARG((int64_t)N * H * W < 2147483648LL, "%s: 2^31 pixels or more", who);
    CVK_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity must be 4 or 8, got %d", who, connectivity);
    return CVK_OK;
}

}  // namespace

// workspace: parents int32 [M] | code bytes [M] | votes int32 [M][num_classes], each part starting on a multiple of 16 bytes
extern "C" int64_t cvk_cc_workspace_bytes(int N, int H, int W, int num_classes) {
    if (!cc_sizes_ok(N, H, W, num_classes)) return 0;
    const int64_t M = (int64_t)N * H * W;
    return cc_round16(4 * M) + cc_round16(M) + 4 * M * num_classes;
}

extern "C" int cvk_cc_record_slots(void) { return CC_RECORD_SLOTS; }

extern "C" int cvk_cc_label(const int64_t* map, int32_t* labels, int32_t* area, int N, int H, int W, int num_classes, int ignore_index,
                            int connectivity, void* workspace, void* stream) {
    CVK_CHECK_ARG(map && labels && area && workspace, "cvk_cc_label: null pointer");
    const int rc = cc_check("cvk_cc_label", N, H, W, num_classes, connectivity);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(labels != area, "cvk_cc_label: labels and area are one buffer");
    hipStream_t s = (hipStream_t)stream;
    const int M = N * H * W, HW = H * W, conn8 = connectivity == 8;
    int* parent = static_cast<int*>(workspace);
    unsigned char* codes = static_cast<unsigned char*>(workspace) + cc_round16(4 * (int64_t)M);
    const int tiles_x = cvk_cdiv(W, CC_TW), tiles_y = cvk_cdiv(H, CC_TH);
    CVK_CHECK_ARG((int64_t)N * tiles_x * tiles_y < 2147483648LL, "cvk_cc_label: too many tiles");
    hipLaunchKernelGGL(k_cc_tile, dim3((unsigned)N * tiles_x * tiles_y), dim3(256), 0, s, map, parent, codes, area, H, W, tiles_x, tiles_y,
                       num_classes, ignore_index, conn8);
    const int64_t total_h = (int64_t)N * (tiles_y - 1) * W, total_v = (int64_t)N * (tiles_x - 1) * H;      // below M / 32 + M / 64
    if (total_h + total_v > 0)
        hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)cvk_cdiv(total_h + total_v, 256)), dim3(256), 0, s, parent, codes, H, W, tiles_y - 1,
                           tiles_x - 1, (int)total_h, (int)total_v, conn8);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)cvk_cdiv(M, 256)), dim3(256), 0, s, parent, labels, area, M, HW);
    hipLaunchKernelGGL(k_cc_area, dim3((unsigned)cvk_cdiv(M, 256)), dim3(256), 0, s, labels, area, M, HW);
    CVK_LAUNCH_RETURN("cvk_cc_label");
}

extern "C" int cvk_cc_filter(const int64_t* map, const int32_t* labels, const int32_t* area, int64_t* out, int64_t* record, int N, int H,
                             int W, int num_classes, int ignore_index, int connectivity, int min_area, int mode, int64_t fill_value,
                             void* workspace, void* stream) {
    CVK_CHECK_ARG(map && labels && area && out && workspace, "cvk_cc_filter: null pointer");
    const int rc = cc_check("cvk_cc_filter", N, H, W, num_classes, connectivity);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(min_area >= 1, "cvk_cc_filter: min_area must be at least 1, got %d", min_area);
    CVK_CHECK_ARG(mode == 0 || mode == 1, "cvk_cc_filter: mode must be 0 (fill) or 1 (neighbour), got %d", mode);
    const int M = N * H * W, HW = H * W, K = num_classes;
    {
        const uintptr_t a = (uintptr_t)map, b = (uintptr_t)out, len = (uintptr_t)M * 8u;
        CVK_CHECK_ARG(a + len <= b || b + len <= a, "cvk_cc_filter: out must not alias map");
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned char* codes = static_cast<unsigned char*>(workspace) + cc_round16(4 * (int64_t)M);
    int* votes = reinterpret_cast<int*>(codes + cc_round16(M));
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(record);
    const int per_image = cvk_cdiv(HW, CC_BLOCK_PIXELS);
    CVK_CHECK_ARG((int64_t)N * per_image < 2147483648LL, "cvk_cc_filter: too many blocks");
    const int64_t v = fill_value;
    const int fill_code = (v >= 0 && v < K && v != (int64_t)ignore_index) ? (int)v : CC_VOID;
    if (mode == 1 || rec)
        hipLaunchKernelGGL(k_cc_prep, dim3((unsigned)N * per_image), dim3(256), 0, s, map, labels, area, codes, mode == 1 ? votes : nullptr, rec,
                           HW, K, ignore_index, min_area, per_image);
    if (mode == 1)
        hipLaunchKernelGGL(k_cc_vote, dim3((unsigned)cvk_cdiv(M, 256)), dim3(256), 0, s, codes, labels, area, votes, M, H, W, K, min_area,
                           connectivity == 8);
    hipLaunchKernelGGL(k_cc_apply, dim3((unsigned)N * per_image), dim3(256), 0, s, map, labels, area, votes, out, rec, HW, K, ignore_index,
                       min_area, mode, fill_value, fill_code, per_image);
    CVK_LAUNCH_RETURN("cvk_cc_filter");
}
