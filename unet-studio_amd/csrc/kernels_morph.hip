// Binary morphology on bit-packed masks (include/unet_morph.h): a mask is uint64[D][H][WPL], voxel x of a line is bit (x & 63) of
// word (x >> 6), and every kernel that writes a mask leaves the bits at and above W zero.
//
//   k_morph_mark     flags[v] = 1 for the listed classes (the host list travels in the kernel arguments, as k_cmp_mark's)
//   k_morph_pack     a wave takes the 64 consecutive x of one word: its ballot of "the label is a listed class" is the word
//   k_morph_unpack   a wave takes a word: lane i writes bit i as a byte
//   k_morph_count    a population count of the valid bits: a sum per wave, one integer add per wave
//   k_morph_copy     iterations == 0: the words, with the bits at and above W cleared
//   step             both kernels work in the "dilation domain": a dilation reads the mask as it is with 0 outside the grid; an
//                    erosion reads the complement with !border outside, dilates that, and complements on the way out.  A loaded
//                    word has its bits at and above W replaced by the outside value, a stored word has them cleared.
//                    morph_nb<CONN> ORs the rows (dy, dz) a connectivity reaches: with a = |dy| + |dz| and a budget of 1, 2, 3 for
//                    6, 18, 26, a row with a <= budget contributes its word, and, when budget - a >= 1, also the word shifted by
//                    one bit either way with the carry bits of the two adjacent words
//   k_morph_step_global   GLOBAL: one thread per output word, the words read from global memory; one launch per iteration
//   k_morph_step_lds      LDS: a block owns a brick of BXW words x BY x BZ rows; it loads the brick with a halo of K rows in y and
//                    z and one word in x, runs K iterations between two LDS copies (iteration i computes the rows at least i inside
//                    the loaded region; a cell outside the grid is put back to the outside value) and stores the brick.  The x
//                    halo word has no neighbour of its own, so after i iterations its i outermost bits are wrong: they are i <= 4
//                    bits away from the brick and never reach it
//   holes
//   k_morph_background    the complement as a uint16 map: 1 where the bit is 0 (a wave per word)
//   launch_components_label   kernels_components.hip: parent[v] = the smallest linear index of v's 6-connected background
//                    component or -1, count[root] = its voxels (below 2^31: bit 31 is spare)
//   k_morph_faces    every voxel on one of the six faces: count[parent[v]] |= bit 31 (a relaxed read first: one atomic OR per root
//                    in the common case)
//   k_morph_holes    a wave per word: the ballot of "parent[v] >= 0 and its root is unmarked" ORed into the input word; info adds
//                    up those voxels and the unmarked roots, one integer add per wave
//   k_morph_apply    a wave per word, the word read once for its 64 voxels of the uint16 label map; changed: one add per wave
// Integer and bitwise arithmetic and integer atomics only; no loop waits for another thread, and every trip count is known at launch.
//
// Scratch, each part 256-B aligned: one mask (the step's other side), the flags of pack uint8[65536], the background map
// uint16[S], the labelling's scratch (components_scratch_bytes(S, 2)).
#include <stdexcept>
#include <string>

#include "../../include/unet_morph.h"
#include "cc_union_find.h"
#include "device_util.h"

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int MORPH_T = 256;          // threads per block: four waves, a wave per word in the per-voxel kernels
constexpr int MORPH_WAVES = MORPH_T / 64;
constexpr int MORPH_MAXB = 4096;      // grid cap of the kernels that add up: they stride over the rest
constexpr int MORPH_CHUNK = 512;      // list entries per k_morph_mark launch (2 KB of kernel arguments)
constexpr int MORPH_FLAGS = 65536;    // n_classes <= 65536
constexpr int BXW = UNET_MORPH_BRICK_XW, BY = UNET_MORPH_BRICK_Y, BZ = UNET_MORPH_BRICK_Z, FUSE = UNET_MORPH_FUSE_MAX;
constexpr int LXW = BXW + 2;          // words of an LDS row: the brick's and one halo word either side
constexpr int LDS_WORDS = LXW * (BY + 2 * FUSE) * (BZ + 2 * FUSE);
constexpr unsigned TOUCHED = 0x80000000u;
static_assert(2 * LDS_WORDS * 8 <= 64 * 1024, "the two LDS copies of a brick with its halo");
static_assert(FUSE >= 1 && FUSE < 64, "a halo word's wrong bits must not reach the brick");

size_t morph_align(size_t b) { return (b + 255) & ~(size_t)255; }

void morph_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("unet_morph: ") + what + ": " + hipGetErrorString(e));
}

struct Scratch {
    u64* mask;
    uint8_t* flags;
    uint16_t* background;
    void* labelling;
};
Scratch morph_scratch(void* scratch, int64_t words, int64_t S) {
    char* b = (char*)morph_align((size_t)(uintptr_t)scratch);   // any scratch alignment: 256 B of slack
    Scratch s;
    s.mask = (u64*)b;
    s.flags = (uint8_t*)(b + morph_align((size_t)words * 8));
    s.background = (uint16_t*)(s.flags + MORPH_FLAGS);
    s.labelling = (char*)s.background + morph_align((size_t)S * 2);
    return s;
}

int64_t morph_wpl(int W) { return ((int64_t)W + 63) / 64; }
// the bits below W of a line's last word
u64 morph_tail(int W) { return (W & 63) ? (((u64)1 << (W & 63)) - 1) : ~(u64)0; }

unsigned morph_word_blocks(int64_t words) { return (unsigned)((words + MORPH_WAVES - 1) / MORPH_WAVES); }   // <= 2^29
unsigned morph_capped(int64_t n, int per_block) {
    const int64_t nb = (n + per_block - 1) / per_block;
    return (unsigned)(nb > MORPH_MAXB ? MORPH_MAXB : nb < 1 ? 1 : nb);
}

struct ListChunk {
    uint32_t v[MORPH_CHUNK];
};

__global__ void __launch_bounds__(MORPH_T) k_morph_mark(uint8_t* __restrict__ flags, ListChunk chunk, int n) {
    for (int i = threadIdx.x; i < n; i += MORPH_T) flags[chunk.v[i]] = 1;   // entries are checked on the host: 0 < v < n_classes
}

// a label of 1 or 2 bytes at any alignment
template <int BYTES>
__device__ __forceinline__ unsigned morph_label(const uint8_t* __restrict__ p, int64_t i) {
    if constexpr (BYTES == 1) return p[i];
    else return (unsigned)p[2 * i] | ((unsigned)p[2 * i + 1] << 8);
}

// the word a wave owns: blocks of MORPH_WAVES waves over the words; false for a whole wave past the end
__device__ __forceinline__ bool morph_wave_word(int64_t words, int wpl, int64_t& word, int& xw, int64_t& line) {
    word = (int64_t)blockIdx.x * MORPH_WAVES + (threadIdx.x >> 6);
    if (word >= words) return false;
    line = word / wpl;
    xw = (int)(word - line * wpl);
    return true;
}

template <int BYTES>
__global__ void __launch_bounds__(MORPH_T) k_morph_pack(int W, int wpl, int64_t words, const uint8_t* __restrict__ labels, int n_classes,
                                                        const uint8_t* __restrict__ flags, u64* __restrict__ bits) {
    int64_t word, line;
    int xw;
    if (!morph_wave_word(words, wpl, word, xw, line)) return;   // wave-uniform: whole waves reach the ballot
    const int lane = threadIdx.x & 63, x = xw * 64 + lane;
    bool member = false;
    if (x < W) {
        const unsigned u = morph_label<BYTES>(labels, line * W + x);
        member = (int)u < n_classes && flags[u];
    }
    const u64 b = __ballot(member);
    if (lane == 0) bits[word] = b;
}

__global__ void __launch_bounds__(MORPH_T) k_morph_unpack(int W, int wpl, int64_t words, const u64* __restrict__ bits,
                                                          uint8_t* __restrict__ mask) {
    int64_t word, line;
    int xw;
    if (!morph_wave_word(words, wpl, word, xw, line)) return;
    const int lane = threadIdx.x & 63, x = xw * 64 + lane;
    if (x < W) mask[line * W + x] = (uint8_t)((bits[word] >> lane) & 1);
}

// sum over the wave, then one add by lane 0
__device__ __forceinline__ void morph_wave_add(u64* dst, u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__global__ void __launch_bounds__(MORPH_T) k_morph_count(int wpl, int64_t words, u64 tail, const u64* __restrict__ bits,
                                                         u64* __restrict__ count) {
    u64 n = 0;
    for (int64_t i = (int64_t)blockIdx.x * MORPH_T + threadIdx.x; i < words; i += (int64_t)gridDim.x * MORPH_T) {
        u64 w = bits[i];
        if ((int)(i % wpl) == wpl - 1) w &= tail;
        n += (u64)__popcll(w);
    }
    morph_wave_add(count, n);
}

__global__ void __launch_bounds__(MORPH_T) k_morph_copy(int wpl, int64_t words, u64 tail, const u64* __restrict__ in,
                                                        u64* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MORPH_T + threadIdx.x;
    if (i >= words) return;
    u64 w = in[i];
    if ((int)(i % wpl) == wpl - 1) w &= tail;
    out[i] = w;
}

// ---- step ------------------------------------------------------------------------------------------------------------------------
// get(dy, dz, dx): the word of the dilation domain at that offset from the output word
template <int CONN, typename Get>
__device__ __forceinline__ u64 morph_nb(Get get) {
    constexpr int budget = CONN == 6 ? 1 : CONN == 18 ? 2 : 3;
    u64 r = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int a = (dy != 0) + (dz != 0);
            if (a > budget) continue;
            const u64 c = get(dy, dz, 0);
            r |= c;
            if (budget - a >= 1) r |= (c << 1) | (c >> 1) | (get(dy, dz, -1) >> 63) | (get(dy, dz, 1) << 63);
        }
    }
    return r;
}

struct StepArgs {
    int wpl, H, D;
    u64 tail;    // the bits below W of a line's last word
    u64 fill;    // the dilation domain outside the grid: all zeros or all ones
    int comp;    // erosion: complement on the way in and on the way out
};

// the word (xw, y, z) of the dilation domain; outside the grid the fill
__device__ __forceinline__ u64 morph_load(const StepArgs& a, const u64* __restrict__ in, int xw, int y, int z) {
    if (xw < 0 || xw >= a.wpl || y < 0 || y >= a.H || z < 0 || z >= a.D) return a.fill;
    u64 v = in[((int64_t)z * a.H + y) * a.wpl + xw];
    if (a.comp) v = ~v;
    if (xw == a.wpl - 1) v = (v & a.tail) | (a.fill & ~a.tail);
    return v;
}

__device__ __forceinline__ void morph_store(const StepArgs& a, u64* __restrict__ out, int xw, int y, int z, u64 v) {
    if (a.comp) v = ~v;
    if (xw == a.wpl - 1) v &= a.tail;
    out[((int64_t)z * a.H + y) * a.wpl + xw] = v;
}

template <int CONN>
__global__ void __launch_bounds__(MORPH_T) k_morph_step_global(StepArgs a, int64_t words, const u64* __restrict__ in, u64* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MORPH_T + threadIdx.x;
    if (i >= words) return;
    const int64_t line = i / a.wpl;
    const int xw = (int)(i - line * a.wpl), y = (int)(line % a.H), z = (int)(line / a.H);
    const u64 r = morph_nb<CONN>([&](int dy, int dz, int dx) { return morph_load(a, in, xw + dx, y + dy, z + dz); });
    morph_store(a, out, xw, y, z, r);
}

// nbx, nby: bricks along x and y.  K iterations; the loaded region is LXW x (BY + 2K) x (BZ + 2K) words
template <int CONN, int K>
__global__ void __launch_bounds__(MORPH_T) k_morph_step_lds(StepArgs a, int nbx, int nby, const u64* __restrict__ in, u64* __restrict__ out) {
    constexpr int LY = BY + 2 * K, LZ = BZ + 2 * K, N = LXW * LY * LZ;
    __shared__ u64 buf[2][LDS_WORDS];
    const unsigned b = blockIdx.x;
    const int xw0 = (int)(b % nbx) * BXW - 1, y0 = (int)((b / nbx) % nby) * BY - K, z0 = (int)(b / ((unsigned)nbx * nby)) * BZ - K;
    for (int l = threadIdx.x; l < N; l += MORPH_T) {
        const int lx = l % LXW, ly = (l / LXW) % LY, lz = l / (LXW * LY);
        buf[0][l] = morph_load(a, in, xw0 + lx, y0 + ly, z0 + lz);
    }
    __syncthreads();
#pragma unroll
    for (int it = 1; it <= K; ++it) {
        const u64* __restrict__ src = buf[(it - 1) & 1];
        u64* __restrict__ dst = buf[it & 1];
        const int ny = LY - 2 * it, nz = LZ - 2 * it, n = LXW * ny * nz;   // the rows at least `it` inside
        for (int j = threadIdx.x; j < n; j += MORPH_T) {
            const int lx = j % LXW, ly = (j / LXW) % ny + it, lz = j / (LXW * ny) + it;
            const int l = (lz * LY + ly) * LXW + lx;
            const int xw = xw0 + lx, y = y0 + ly, z = z0 + lz;
            u64 r;
            if (xw < 0 || xw >= a.wpl || y < 0 || y >= a.H || z < 0 || z >= a.D) {
                r = a.fill;                                            // the outside never changes
            } else {
                r = morph_nb<CONN>([&](int dy, int dz, int dx) {
                    const int xx = lx + dx;
                    return xx < 0 || xx >= LXW ? (u64)0 : src[l + (dz * LY + dy) * LXW + dx];
                });
                if (xw == a.wpl - 1) r = (r & a.tail) | (a.fill & ~a.tail);
            }
            dst[l] = r;
        }
        __syncthreads();
    }
    const u64* __restrict__ res = buf[K & 1];
    for (int j = threadIdx.x; j < BXW * BY * BZ; j += MORPH_T) {
        const int lx = j % BXW + 1, ly = (j / BXW) % BY + K, lz = j / (BXW * BY) + K;
        const int xw = xw0 + lx, y = y0 + ly, z = z0 + lz;
        if (xw < a.wpl && y < a.H && z < a.D) morph_store(a, out, xw, y, z, res[(lz * LY + ly) * LXW + lx]);
    }
}

template <int CONN>
void morph_launch_lds(int k, const StepArgs& a, int nbx, int nby, unsigned blocks, const u64* in, u64* out, hipStream_t s) {
    switch (k) {
        case 1: k_morph_step_lds<CONN, 1><<<blocks, MORPH_T, 0, s>>>(a, nbx, nby, in, out); break;
        case 2: k_morph_step_lds<CONN, 2><<<blocks, MORPH_T, 0, s>>>(a, nbx, nby, in, out); break;
        case 3: k_morph_step_lds<CONN, 3><<<blocks, MORPH_T, 0, s>>>(a, nbx, nby, in, out); break;
        default: k_morph_step_lds<CONN, 4><<<blocks, MORPH_T, 0, s>>>(a, nbx, nby, in, out); break;
    }
}
static_assert(FUSE == 4, "morph_launch_lds instantiates K = 1..4");

// ---- holes -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MORPH_T) k_morph_background(int W, int wpl, int64_t words, const u64* __restrict__ bits,
                                                              uint16_t* __restrict__ background) {
    int64_t word, line;
    int xw;
    if (!morph_wave_word(words, wpl, word, xw, line)) return;
    const int lane = threadIdx.x & 63, x = xw * 64 + lane;
    if (x < W) background[line * W + x] = (uint16_t)(((bits[word] >> lane) & 1) ^ 1);
}

// the voxels of the six faces, one section per axis (edges and corners come more than once)
__global__ void __launch_bounds__(MORPH_T) k_morph_faces(int W, int H, int D, const int* __restrict__ parent, unsigned* __restrict__ count) {
    const int64_t A = 2 * (int64_t)H * D, B = 2 * (int64_t)W * D, total = A + B + 2 * (int64_t)W * H;
    for (int64_t idx = (int64_t)blockIdx.x * MORPH_T + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * MORPH_T) {
        int x, y, z;
        if (idx < A) {
            int64_t j = idx;
            x = (j & 1) ? W - 1 : 0; j >>= 1;
            y = (int)(j % H); z = (int)(j / H);
        } else if (idx < A + B) {
            int64_t j = idx - A;
            y = (j & 1) ? H - 1 : 0; j >>= 1;
            x = (int)(j % W); z = (int)(j / W);
        } else {
            int64_t j = idx - A - B;
            z = (j & 1) ? D - 1 : 0; j >>= 1;
            x = (int)(j % W); y = (int)(j / W);
        }
        const int r = parent[((int64_t)z * H + y) * W + x];
        if (r < 0) continue;
        // the bit is only ever set: a root seen marked needs no atomic
        if (!(__hip_atomic_load(count + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & TOUCHED)) atomicOr(count + r, TOUCHED);
    }
}

__global__ void __launch_bounds__(MORPH_T) k_morph_holes(int W, int wpl, int64_t words, u64 tail, const u64* in,
                                                         const int* __restrict__ parent, const unsigned* __restrict__ count, u64* out,
                                                         u64* __restrict__ info) {   // in may be out: a word is read, then written, by one lane
    int64_t word, line;
    int xw;
    if (!morph_wave_word(words, wpl, word, xw, line)) return;   // wave-uniform
    const int lane = threadIdx.x & 63, x = xw * 64 + lane;
    bool hole = false, root = false;
    if (x < W) {
        const int64_t v = line * W + x;
        const int r = parent[v];
        hole = r >= 0 && !(count[r] & TOUCHED);
        root = hole && r == (int)v;
    }
    const u64 hb = __ballot(hole), rb = __ballot(root);
    if (lane == 0) {
        u64 w = in[word];
        if (xw == wpl - 1) w &= tail;
        out[word] = w | hb;
        if (info) {
            if (hb) atomicAdd(info, (u64)__popcll(hb));
            if (rb) atomicAdd(info + 1, (u64)__popcll(rb));
        }
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(MORPH_T) k_morph_apply(int W, int wpl, int64_t words, uint16_t* __restrict__ labels,
                                                         const u64* __restrict__ bits, uint16_t value, u64* __restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int64_t first = (int64_t)blockIdx.x * MORPH_WAVES + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * MORPH_WAVES;
    u64 n = 0;
    for (int64_t word = first; word < words; word += stride) {   // wave-uniform
        const int64_t line = word / wpl;
        const int x = (int)(word - line * wpl) * 64 + lane;
        if (x >= W) continue;
        const bool bit = (bits[word] >> lane) & 1;
        uint16_t* p = labels + line * W + x;
        const uint16_t u = *p;
        if (MODE == UNET_MORPH_SET ? (bit && u == 0) : (!bit && u == value)) {
            *p = MODE == UNET_MORPH_SET ? value : (uint16_t)0;
            ++n;
        }
    }
    if (changed) morph_wave_add(changed, n);
}

}  // namespace

size_t morph_scratch_bytes(int W, int H, int D) {
    const int64_t S = (int64_t)W * H * D, words = morph_wpl(W) * H * D;
    return 256 + morph_align((size_t)words * 8) + MORPH_FLAGS + morph_align((size_t)S * 2) + components_scratch_bytes(S, 2);
}

// classes: n entries in (0, n_classes), host memory; read before this returns
void launch_morph_pack(int W, int H, int D, const void* labels, int label_bytes, int n_classes, const uint32_t* classes, int n,
                       uint64_t* bits, void* scratch, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D;
    if (n == 0) {
        morph_check(hipMemsetAsync(bits, 0, (size_t)words * 8, s), "hipMemsetAsync");
        return;
    }
    const Scratch sc = morph_scratch(scratch, words, (int64_t)W * H * D);
    morph_check(hipMemsetAsync(sc.flags, 0, MORPH_FLAGS, s), "hipMemsetAsync");
    for (int c0 = 0; c0 < n; c0 += MORPH_CHUNK) {
        ListChunk chunk;
        const int m = n - c0 < MORPH_CHUNK ? n - c0 : MORPH_CHUNK;
        for (int i = 0; i < MORPH_CHUNK; ++i) chunk.v[i] = i < m ? classes[c0 + i] : 0u;
        k_morph_mark<<<1, MORPH_T, 0, s>>>(sc.flags, chunk, m);
    }
    const unsigned nb = morph_word_blocks(words);
    if (label_bytes == 1)
        k_morph_pack<1><<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, (const uint8_t*)labels, n_classes, sc.flags, (u64*)bits);
    else
        k_morph_pack<2><<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, (const uint8_t*)labels, n_classes, sc.flags, (u64*)bits);
}

void launch_morph_unpack(int W, int H, int D, const uint64_t* bits, uint8_t* mask, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D;
    k_morph_unpack<<<morph_word_blocks(words), MORPH_T, 0, s>>>(W, (int)wpl, words, (const u64*)bits, mask);
}

void launch_morph_count(int W, int H, int D, const uint64_t* bits, int64_t* count, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D;
    morph_check(hipMemsetAsync(count, 0, 8, s), "hipMemsetAsync");
    k_morph_count<<<morph_capped(words, MORPH_T), MORPH_T, 0, s>>>((int)wpl, words, morph_tail(W), (const u64*)bits, (u64*)count);
}

// impl: UNET_MORPH_IMPL_LDS or _GLOBAL (the caller resolves DEFAULT)
void launch_morph_step(int W, int H, int D, const uint64_t* in, uint64_t* out, int op, int connectivity, int iterations, int border,
                       int impl, void* scratch, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D;
    const unsigned nb = (unsigned)((words + MORPH_T - 1) / MORPH_T);
    if (iterations == 0) {
        k_morph_copy<<<nb, MORPH_T, 0, s>>>((int)wpl, words, morph_tail(W), (const u64*)in, (u64*)out);
        return;
    }
    StepArgs a;
    a.wpl = (int)wpl; a.H = H; a.D = D;
    a.tail = morph_tail(W);
    a.comp = op == UNET_MORPH_ERODE;
    a.fill = a.comp && !border ? ~(u64)0 : (u64)0;   // an erosion's outside reads !border in the complement
    const Scratch sc = morph_scratch(scratch, words, (int64_t)W * H * D);
    const bool lds = impl == UNET_MORPH_IMPL_LDS;
    const int launches = lds ? (iterations + FUSE - 1) / FUSE : iterations;
    const int nbx = (int)((wpl + BXW - 1) / BXW), nby = (H + BY - 1) / BY, nbz = (D + BZ - 1) / BZ;   // nbx * nby * nbz <= words
    const u64* src = (const u64*)in;
    int left = iterations;
    for (int j = 1; j <= launches; ++j) {
        u64* dst = (launches - j) % 2 == 0 ? (u64*)out : sc.mask;   // alternate so that the last launch writes out
        if (lds) {
            const int k = left < FUSE ? left : FUSE;
            const unsigned blocks = (unsigned)nbx * nby * nbz;
            if (connectivity == 6) morph_launch_lds<6>(k, a, nbx, nby, blocks, src, dst, s);
            else if (connectivity == 18) morph_launch_lds<18>(k, a, nbx, nby, blocks, src, dst, s);
            else morph_launch_lds<26>(k, a, nbx, nby, blocks, src, dst, s);
            left -= k;
        } else {
            if (connectivity == 6) k_morph_step_global<6><<<nb, MORPH_T, 0, s>>>(a, words, src, dst);
            else if (connectivity == 18) k_morph_step_global<18><<<nb, MORPH_T, 0, s>>>(a, words, src, dst);
            else k_morph_step_global<26><<<nb, MORPH_T, 0, s>>>(a, words, src, dst);
        }
        src = dst;
    }
}

// labelling: UNET_COMPONENTS_IMPL_*; connectivity: the background's, 6, 18 or 26
void launch_morph_holes(int W, int H, int D, const uint64_t* in, uint64_t* out, int64_t* info, int labelling, int connectivity,
                        void* scratch, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D, S = (int64_t)W * H * D;
    const Scratch sc = morph_scratch(scratch, words, S);
    if (info) morph_check(hipMemsetAsync(info, 0, 16, s), "hipMemsetAsync");
    const unsigned nb = morph_word_blocks(words);
    k_morph_background<<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, (const u64*)in, sc.background);
    const uint32_t one = 1;
    const ComponentsForest f = launch_components_label(W, H, D, sc.background, 2, &one, 1, labelling, connectivity, sc.labelling, s);
    const int64_t faces = 2 * ((int64_t)H * D + (int64_t)W * D + (int64_t)W * H);
    k_morph_faces<<<morph_capped(faces, MORPH_T), MORPH_T, 0, s>>>(W, H, D, f.parent, f.count);
    k_morph_holes<<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, morph_tail(W), (const u64*)in, f.parent, f.count, (u64*)out, (u64*)info);
}

void launch_morph_apply(int W, int H, int D, uint16_t* labels, const uint64_t* bits, int value, int mode, int64_t* changed, hipStream_t s) {
    const int64_t wpl = morph_wpl(W), words = wpl * H * D;
    if (changed) morph_check(hipMemsetAsync(changed, 0, 8, s), "hipMemsetAsync");
    const unsigned nb = morph_capped(words, MORPH_WAVES);
    if (mode == UNET_MORPH_SET)
        k_morph_apply<UNET_MORPH_SET><<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, labels, (const u64*)bits, (uint16_t)value, (u64*)changed);
    else
        k_morph_apply<UNET_MORPH_KEEP><<<nb, MORPH_T, 0, s>>>(W, (int)wpl, words, labels, (const u64*)bits, (uint16_t)value, (u64*)changed);
}

}  // namespace unet
