// sz_nn_common.h — device helpers shared by the network kernels (sz_nn.hip: bf16 tower, heads, per-layer kernels; sz_nn_split.hip: the
// split-precision tower): vector types, bf16 packing, LDS staging of the input planes, the weight-fragment stream through a buffer
// descriptor, the position-tile / tap-address mapping of the 16x16x32 MFMA path, and the host-side launch plumbing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include "../../include/sigmazero.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define NN_COUT 256
#define NN_NI 2                                            // channel tiles (32) per wave of the 32x32x16 kernels
#define NN_PAD16 32                                        // LDS row padding of the 16x16x32 path (bytes)
#define NN_ZERO16 768                                      // zero region behind the rows of a 16x16x32-path image (see conv_kloop16 tap_addr)

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) short i16x2;
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));       // ONE v_cvt_pk_bf16_f32 (round-to-nearest-even)
}
// ReLU on a packed bf16 pair: a negative bf16 is a negative int16, so max(x, 0) per 16-bit half is the ReLU (v_pk_max_i16; -0 -> +0)
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t x) {
    i16x2 v = __builtin_bit_cast(i16x2, x), z = {0, 0};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(v, z));
}
__device__ __forceinline__ float bf16_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xFFFF0000u); }

// ---- operand element of the 16x16x32 MFMA path: bf16 (8 bits of mantissa, f32's range) or f16 (11 bits, range 6e-5 .. 65504: post-BatchNorm
// activations and BatchNorm-folded weights are O(1), comfortably inside).  Same MFMA cycles, same LDS / weight bytes, one pack instruction per pair either
// way (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32, both round to nearest even), two to expand a pair; ReLU on the packed pair is v_pk_max_i16 for both (sign bit).
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
struct ElemBF16 {
    static constexpr uint32_t ONE = 0x3F80u;
    static __device__ __forceinline__ uint32_t pack2(float a, float b) { return pack_bf16x2(a, b); }
    static __device__ __forceinline__ float lo(uint32_t v) { return bf16_lo(v); }
    static __device__ __forceinline__ float hi(uint32_t v) { return bf16_hi(v); }
    static __device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static uint16_t from_float(float v) { uint32_t u; memcpy(&u, &v, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }      // host, RNE (finite input)
};
struct ElemF16 {
    static constexpr uint32_t ONE = 0x3C00u;
    static __device__ __forceinline__ uint32_t pack2(float a, float b) { f32x2 v = {a, b}; return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2)); }
    static __device__ __forceinline__ float lo(uint32_t v) { return (float)__builtin_bit_cast(f16x2, v)[0]; }
    static __device__ __forceinline__ float hi(uint32_t v) { return (float)__builtin_bit_cast(f16x2, v)[1]; }
    static __device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    static uint16_t from_float(float v) { const _Float16 h = (_Float16)v; uint16_t u; memcpy(&u, &h, 2); return u; }                          // host, RNE
};

// A value written by v_accvgpr_write has an AGPR-class live range: it stays in the accumulator file across a K loop instead of taking a vector register there.
__device__ __forceinline__ float to_agpr(float v) { float a; asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v)); return a; }
__device__ __forceinline__ float from_agpr(float a) { float v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; }

// exp(d), d = logit - row maximum <= 0, of the three softmax epilogues (k_policy_head, k_heads16_bf16, split_heads_tail).  __expf is one multiply by log2(e) and one
// v_exp_f32, and v_exp_f32 delivers no subnormal result: everything below 2^-126 (d < -87.34) came out as 0, where torch's fp32 softmax keeps f32's subnormals
// down to d = -103.97, and the search keeps a child iff its probability is not 0.  exp2f on the same product is the same v_exp_f32 from 2^-126 up (bit for bit
// what __expf gave); below, the exponential is taken 2^64 higher (the + 64 is exact: the product's quantum is at least the sum's) and scaled down by one
// v_ldexp_f32, which rounds once into the subnormal range.
__device__ __forceinline__ float softmax_exp(float d) { return exp2f(d * 1.44269504088896340736f); }

// ---- f16 range tracking (ElemF16 epilogues only; the bf16 instantiations carry none of it) ---------------------------------------------------------------
// A stored activation of 65520 or more packs to +inf, the next convolution makes NaN of it (inf - inf), and the integer ReLU erases a NaN whose sign bit is set:
// the overflow can leave a launch as finite garbage.  So it is remembered where it is created: AFTER the ReLU both halves of a packed pair are >= +0 as int16 and
// inf / NaN are exactly the patterns from 0x7C00 up, so a running per-half integer maximum (v_pk_max_i16) of everything a lane stored tells at the end of the
// kernel whether a stored value had left the range.  The running maximum lives in an AGPR (read, max, write back per stored tile): the tower kernels have no
// vector register to spare across their K loops (kept in a VGPR it was spilled to scratch around every update).  A value of -65520 or below packs to -inf and the
// ReLU makes the 0 of it that the exact value gives too: no overflow.
struct RangeSeen { float a; };                             // the AGPR-resident running maximum (bit pattern of two int16)
__device__ __forceinline__ RangeSeen range_none() { RangeSeen r; r.a = to_agpr(0.f); return r; }
template <class E> __device__ __forceinline__ void range_track(RangeSeen& seen, uint32_t pair0, uint32_t pair1) {           // the two pairs of one stored tile, after the ReLU
    if constexpr (std::is_same<E, ElemF16>::value) {
        const i16x2 m = __builtin_elementwise_max(__builtin_elementwise_max(__builtin_bit_cast(i16x2, pair0), __builtin_bit_cast(i16x2, pair1)),
                                                  __builtin_bit_cast(i16x2, from_agpr(seen.a)));
        seen.a = to_agpr(__builtin_bit_cast(float, m));
    }
}
// the same with the running maximum in a plain register (the heads kernel: two workgroups per CU, no accumulator file of its own)
template <class E> __device__ __forceinline__ void range_track(uint32_t& seen, uint32_t pair0, uint32_t pair1) {
    if constexpr (std::is_same<E, ElemF16>::value)
        seen = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_elementwise_max(__builtin_bit_cast(i16x2, pair0), __builtin_bit_cast(i16x2, pair1)),
                                                                      __builtin_bit_cast(i16x2, seen)));
}
template <class E> __device__ __forceinline__ void range_report(uint32_t m, unsigned int* flag) {
    if constexpr (std::is_same<E, ElemF16>::value) { if (flag && ((m & 0xFFFFu) >= 0x7C00u || (m >> 16) >= 0x7C00u)) atomicOr(flag, 1u); }
}
// end of a kernel: one vector atomic per lane that saw an overflow (none in a healthy network)
template <class E> __device__ __forceinline__ void range_report(const RangeSeen& seen, unsigned int* flag) {
    if constexpr (std::is_same<E, ElemF16>::value) {
        const uint32_t m = __builtin_bit_cast(uint32_t, from_agpr(seen.a));
        if (flag && ((m & 0xFFFFu) >= 0x7C00u || (m >> 16) >= 0x7C00u)) atomicOr(flag, 1u);
    }
}

// ---- stage WGB boards' activations (NHWC rows of C_in bf16) into LDS, plus the zero region (PAD 16: one zero row) behind them ----
template <int CIN, int WGB, int PAD, bool SWZ = false /* chunk swizzle of the split-precision images: chunk ^ ((position >> 2) & 1) */>
__device__ __forceinline__ void stage_tile(unsigned char* lds, const uint16_t* __restrict__ in, int board0, int n_boards) {
    constexpr int PITCH = CIN * 2 + PAD;
    constexpr int CHUNKS_PER_POS = CIN / 8;                // 16-B chunks per position
    constexpr int TOTAL = WGB * 64 * CHUNKS_PER_POS;
    constexpr int PER_THREAD = TOTAL / 256;
    const int tid = threadIdx.x;
    const uint4* src = (const uint4*)(in + (size_t)board0 * 64 * CIN);
    const int valid_chunks = min(WGB, n_boards - board0) * 64 * CHUNKS_PER_POS;
    // all loads of a thread are issued before the first LDS write (the accumulators are not live yet, so the
    // registers are free) -> one HBM latency per workgroup
    uint4 stage[PER_THREAD];
#pragma unroll
    for (int i = 0; i < PER_THREAD; i++) {
        const int c = tid + i * 256;
        stage[i] = c < valid_chunks ? src[c] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < PER_THREAD; i++) {
        const int c = tid + i * 256;
        *(uint4*)(lds + (c / CHUNKS_PER_POS) * PITCH + ((c % CHUNKS_PER_POS) ^ (SWZ ? ((c / CHUNKS_PER_POS) >> 2) & 1 : 0)) * 16) = stage[i];
    }
    for (int c = tid; c < (PAD == NN_PAD16 ? NN_ZERO16 : PITCH) / 16; c += 256) *(uint4*)(lds + WGB * 64 * PITCH + c * 16) = make_uint4(0, 0, 0, 0);
}

// ---- stage WGB boards from the engine's bit-packed planes (SZ_PLANES_NHWC128_BITS: 1 KiB per board) ----------
// uint4 l of a board (l = psub*16 + cq): byte q = channels cq*8..cq*8+7 of position q*4 + psub.  Two threads share a
// uint4 (q 0..7 / 8..15); each expands 8 bytes to 8 chunks of 8 elements (1.0 = E::ONE) and writes them to its LDS rows.
template <int WGB, int PAD, class E = ElemBF16, bool SWZ = false>
__device__ __forceinline__ void stage_tile_bits(unsigned char* lds, const uint16_t* __restrict__ in, int board0, int n_boards) {
    constexpr int PITCH = 128 * 2 + PAD;
    const uint4* src = (const uint4*)in + (size_t)board0 * 64;
    for (int t = threadIdx.x; t < WGB * 128; t += 256) {
        const int board = t >> 7, half = (t >> 6) & 1, l = t & 63, psub = l >> 4, cq = l & 15;
        uint4 v = (board0 + board < n_boards) ? src[board * 64 + l] : make_uint4(0, 0, 0, 0);
        const uint32_t w0 = half ? v.z : v.x, w1 = half ? v.w : v.y;
#pragma unroll
        for (int qq = 0; qq < 8; qq++) {
            const uint32_t byte = ((qq < 4 ? w0 : w1) >> ((qq & 3) * 8)) & 0xFFu;
            uint4 o;
            o.x = ((byte & 1) ? E::ONE : 0u) | ((byte & 2) ? (E::ONE << 16) : 0u);
            o.y = ((byte & 4) ? E::ONE : 0u) | ((byte & 8) ? (E::ONE << 16) : 0u);
            o.z = ((byte & 16) ? E::ONE : 0u) | ((byte & 32) ? (E::ONE << 16) : 0u);
            o.w = ((byte & 64) ? E::ONE : 0u) | ((byte & 128) ? (E::ONE << 16) : 0u);
            const int pos = (half * 8 + qq) * 4 + psub;
            *(uint4*)(lds + (board * 64 + pos) * PITCH + (cq ^ (SWZ ? (pos >> 2) & 1 : 0)) * 16) = o;
        }
    }
    for (int c = threadIdx.x; c < NN_ZERO16 / 16; c += 256) *(uint4*)(lds + WGB * 64 * PITCH + c * 16) = make_uint4(0, 0, 0, 0);
}

// One weight fragment through a buffer descriptor: UNIFORM base (kernel argument -> 4 SGPRs) + uniform element offset (soffset, SGPR)
// + the lane's constant 32-bit byte offset (voffset, one VGPR).  With flat global_load hipcc carried a 64-bit per-lane pointer per
// weight stream and hoisted a dozen of them out of the tile loop of the persistent tower: those were its 24 spilled VGPRs (100 B/lane of
// scratch, reloaded with vmcnt(0) waits once per tile — never inside a K loop, but serialising the first prefetch of every tile;
// profiles/r02c_tower_stamps_buffer_loads.txt against r02c_tower_stamps_flat_loads.txt).
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
struct WSrc { __amdgpu_buffer_rsrc_t r; };
__device__ __forceinline__ WSrc wfrag_rsrc(const uint4* __restrict__ w) {
    WSrc s;
    s.r = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, 0x7FFFFFFF, 0x00020000);   // raw buffer, no stride; weights of one conv are < 2 MB
    return s;
}
__device__ __forceinline__ uint4 ld_wfrag(const WSrc& s, size_t uniform_off, uint32_t lane_bytes) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(s.r, (int)lane_bytes, (int)(uniform_off * 16), 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Which 16 positions form MFMA position tile j: image row (= board*64 + position) of the tile's column p16.
//   2-board workgroups: tile j = board ROW j of BOTH boards (lanes 0..7 board 0, 8..15 board 1).  Under the three taps that look one row up (dy = -1)
//     tile 0 reads nothing but off-board zeros, under the three that look down tile 7 does: those 6 of 72 tap-tiles are skipped outright
//     (conv_kloop16 SKIPROWS, 8.3 % of the MFMAs).  Eight consecutive lanes still read eight consecutive image rows: ds_read_b128 stays conflict-free.
//   1-board workgroups: tile j = rows 2j, 2j+1 of the board (no tile is ever entirely off the board).
template <int WGB>
__device__ __forceinline__ int tile_row(int j, int p16) {
    if constexpr (WGB == 2) return (p16 >> 3) * 64 + j * 8 + (p16 & 7);
    else return (j >> 2) * 64 + (j & 3) * 16 + p16;
}

// LDS byte offset (inside its image) that lane (p16, kg) reads for position tile j under tap `tap` — see conv_kloop16 for the zero region
// SWZ (the split-precision images): the 16-byte chunk index of a row's data is XOR-ed with bit 2 of the row's position (chunk ^ ((row >> 2) & 1), i.e. the two
// lane quarters kg, kg^1 trade places on rows 4..7 of every 8): it makes the epilogue's ds_write_b128 (8 lanes = 8 consecutive rows at one channel offset)
// conflict-free and leaves ds_read_b128 conflict-free (slot 2*row + (kg ^ g) is still a permutation per lane group).
template <int PITCH, int NTAPS, int WGB, bool SWZ = false>
__device__ __forceinline__ int conv_tap_addr16(int tap, int j, int p16, int kg) {
    const int dy = (NTAPS == 9) ? tap / 3 - 1 : 0, dx = (NTAPS == 9) ? tap % 3 - 1 : 0;
    const int row0 = tile_row<WGB>(j, p16), pos = row0 & 63;   // position inside its board (board = row0 >> 6)
    const int y = (pos >> 3) + dy, x = (pos & 7) + dx;
    const bool ok = (unsigned)y < 8u && (unsigned)x < 8u;
    const int vrow = pos + 8 * dy + dx;
    return ok ? ((row0 >> 6) * 64 + y * 8 + x) * PITCH + (SWZ ? (kg ^ ((x >> 2) & 1)) : kg) * 16 : WGB * 64 * PITCH + ((2 * vrow + kg) & 15) * 16;
}

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { fprintf(stderr, "[sigmazero] HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); return SZ_ERR_HIP; } } while (0)

// the network entry points carry no engine handle: they run on the device that owns the caller's stream (a rank whose current
// device is another GPU would otherwise launch into the wrong context) and restore the caller's current device on return
struct StreamDeviceGuard {
    int prev = -1; bool changed = false;
    explicit StreamDeviceGuard(void* stream) {
        hipDevice_t sd = 0;
        if (!stream || hipStreamGetDevice((hipStream_t)stream, &sd) != hipSuccess) return;     // the null stream belongs to the current device
        if (hipGetDevice(&prev) == hipSuccess && prev != (int)sd) changed = (hipSetDevice((int)sd) == hipSuccess);
    }
    ~StreamDeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

#define NN_MAX_DEVICES 16
static inline int current_device_slot() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev % NN_MAX_DEVICES;
}
static inline int device_cus() {
    static int n_cu[NN_MAX_DEVICES] = {};
    int& n = n_cu[current_device_slot()];
    if (!n) {
        int dev = 0; hipDeviceProp_t prop;
        n = 256;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
    }
    return n;
}
