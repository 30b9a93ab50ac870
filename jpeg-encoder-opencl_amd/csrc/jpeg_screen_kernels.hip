// Screened transform pipeline (gfx950 / CDNA4): the reference's in-place fp64 chain
// evaluated as an exact fixed-point linear map on the int8 MFMA units, with a
// rigorous accept/recompute test so that the results stay bit-identical.
//
// Why this is legal: in exact arithmetic the chain of
// utils.cpp:314-348 is a fixed 64x64 linear map L of the level-shifted samples
// p in [-128,127]^64.  The fp64 chain c the reference runs differs from L p only by
// rounding, |c_k - (L p)_k| <= eps_k (forward error analysis,
// tools/gen_screen_tables.py).  The kernel computes Lt p exactly, Lt = round(L*2^39)
// split into five balanced int8 digits (|Lt - L| p <= 2^-27), so
// |c_k/Q_k - z_k| <= tau_k with z_k = (Lt p)_k / Q_k.  The reference's quantiser
// round(fl(c/Q)) equals round-half-away of the exact quotient, so
// whenever z_k is farther than tau_k from every half-integer the quantised value
// is decided.  Units with an undecided coefficient are recomputed (inside the same kernel,
// exact_unit_wave) with the exact ordered fp64 chain -- that chain remains the arbiter.  Coefficient 0 is
// always exact: row 0 of L is SCALE_00 * ones, so c_0 = fl(sum(p) * SCALE_00) is
// formed directly.
//
// Pipeline per batch:
//   k_screen_encode  RGB -> per-unit {DC, AC bit string (word-aligned blob in an arena)}
//                    samples (integer-exact CSC), MFMA map, quantise+verify, LDS transpose to
//                    zig-zag rows, per-unit RLE/Huffman walk into an LDS slot, blob store
//                    (+ the exact fp64 chain for the rare undecided units)
//   k_dc_heads       DC symbol of each tile's first unit per pass -> tile sums
//   k_tile_scan      (jpeg_kernels.hip) 64-bit scan of tile sums
//   k_merge          DC symbols + AC blobs -> final bit string (LDS window per tile)
// Gray frames (MI355_F_GRAY) run k_gray_encode, k_gray_dc_heads, k_tile_scan, k_gray_merge: the same pipeline with one
// pass per tile.
#include "jpeg_screen_devfn.h"

namespace mi355 {

constexpr uint32_t kEncWaves = 4;

// An error in a unit also poisons its tile's bit total (bit 31, never reached by the sums): k_tile_scan then knows WHICH
// frame failed.
#define POISON_TILE() atomicOr(&sp.tile_bits[(size_t)frame * g.tiles + tile], 0x80000000u)
#define POISON_FT() atomicOr(&sp.tile_bits[ft], 0x80000000u)

// Diagnostic build (make STAMPS=1): s_memtime stamps at the phase boundaries of a wave
// iteration, summed per wave and written to sp.stamps.  Never in the shipped kernel.
#ifdef MI355_STAMPS
#define STAMP(i)                                                                         \
    do {                                                                                 \
        unsigned long long _t;                                                           \
        __builtin_amdgcn_sched_barrier(0);                                               \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");       \
        __builtin_amdgcn_sched_barrier(0);                                               \
        stamp_sum[i] += _t - stamp_prev;                                                 \
        stamp_prev = _t;                                                                 \
    } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// MODE 0: strict (the reference's arithmetic); 1: standard 4:4:4; 2: standard 4:2:0 (tile = 64 MCUs,
// six passes: luma quarter-tiles 0..3 -- unit u of pass s is block k = u & 3 of MCU 16 s + u / 4, i.e.
// the scan order of the luma blocks -- then Cb, Cr with one block per MCU).
// At most 224 registers (the attribute counts in units of two on gfx90a and later: 112): two workgroups of this kernel
// per CU leave 64 per SIMD lane, which is what the tail kernels of the part in front need to run BESIDE it (k_merge: two
// waves, 32 allocated each; one register granule more and batched calls lose a fifth to a quarter: DESIGN.md §4.5,
// tests/test_kernel_budget.py).
template <bool PROBE, int MODE>
__attribute__((amdgpu_num_vgpr(112))) __global__ void __launch_bounds__(256, 2)
    k_screen_encode(Geom g, uint32_t n_frames, const uint8_t* __restrict__ rgb, ScreenParams sp) {
#include "jpeg_screen_encode_body.h"
}

// Gray (MI355_F_GRAY, MODE 3 of the body): one component, one pass per tile, samples straight from the input bytes (W*H
// per frame) -- no colour conversion.  The same register and LDS budget as the forms above, so that the tail kernels of
// a batched call fit beside it the same way (tests/test_gray_kernel_budget.py).
template <bool PROBE>
__attribute__((amdgpu_num_vgpr(112))) __global__ void __launch_bounds__(256, 2)
    k_gray_encode(Geom g, uint32_t n_frames, const uint8_t* __restrict__ rgb, ScreenParams sp) {
    constexpr int MODE = 3;
#include "jpeg_screen_encode_body.h"
}

// ----------------------------------------------------------------------------
// k_dc_heads: DC symbol of the first unit of every (tile, pass).  Its predecessor is the last
// block of the previous tile (or luma quarter-tile), encoded by another wave of k_screen_encode,
// which therefore left the symbol out of the tile sum.  Every DC in `meta` is exact already
// (the exact recomputation keeps coefficient 0).  Light on purpose (few registers, 128 B of LDS): it runs every
// frame next to another stream's k_screen_encode.
// ----------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
    k_dc_heads(Geom g, uint32_t n_frames, ScreenParams sp) {
    __shared__ uint32_t s_dcf[2][16];
    // short kernel on its stream's critical path, usually resident next to another stream's
    // k_screen_encode: do not let it starve behind those (older) waves
    __builtin_amdgcn_s_setprio(3);
    const uint32_t lane = threadIdx.x;
    if (lane < 32) s_dcf[lane >> 4][lane & 15] = sp.lut[(lane >> 4) * 256 + (lane & 15)];
    __syncthreads();
    const uint32_t P = g.passes, heads = n_frames * g.tiles * P;
    const bool restart = (g.flags & 8u) != 0;  // MI355_F_RESTART: DC predictors start from 0 in every tile
    for (uint32_t p = blockIdx.x * 64 + lane; p < heads; p += gridDim.x * 64) {
        const uint32_t ft = p / P, c = p - ft * P, tile = restart ? 0u : ft % g.tiles;
        const size_t u0 = (size_t)p * 64;  // ((frame * tiles + tile) * passes + c) * 64
        int pred = 0;
        bool luma = c == 0;
        if (P == 6) {
            // 4:2:0: luma quarter-tile c follows quarter-tile c - 1 (or the previous tile's quarter-tile 3);
            // a quarter-tile past the last MCU has no units at all
            luma = c < 4;
            if (luma && (ft % g.tiles) * 64 + 16 * c >= g.N) continue;
            if (luma && c > 0) pred = meta_dc(sp.meta[u0 - 64 + 63]);
            else if (tile > 0) pred = meta_dc(sp.meta[u0 - 6 * 64 + (luma ? 3 * 64 : 0) + 63]);
        } else if (tile > 0) {
            pred = meta_dc(sp.meta[u0 - 192 + 63]);
        }
        const int dc = meta_dc(sp.meta[u0]);
        uint32_t len = 0;
        auto count = [&](uint32_t, uint32_t l) { len += l; };
        if (!put_dc(dc - pred, s_dcf[luma ? 0 : 1], count)) atomicOr(sp.status, 1u), POISON_FT();  // MI355_E_CATEGORY
        atomicAdd(&sp.tile_bits[ft], len);
    }
}

// Gray (one pass per tile): the predecessor of a tile's first unit is the last unit of the pass in front.  A kernel of
// its own -- k_dc_heads above reads three passes back -- with the same light footprint.
__global__ void __launch_bounds__(64)
    k_gray_dc_heads(Geom g, uint32_t n_frames, ScreenParams sp) {
    __shared__ uint32_t s_dcl[16];
    __builtin_amdgcn_s_setprio(3);  // see k_dc_heads
    const uint32_t lane = threadIdx.x;
    if (lane < 16) s_dcl[lane] = sp.lut[lane];  // DC luma
    __syncthreads();
    const uint32_t heads = n_frames * g.tiles;
    const bool restart = (g.flags & 8u) != 0;  // MI355_F_RESTART: DC predictors start from 0 in every tile
    for (uint32_t ft = blockIdx.x * 64 + lane; ft < heads; ft += gridDim.x * 64) {
        const uint32_t tile = restart ? 0u : ft % g.tiles;
        const size_t u0 = (size_t)ft * 64;  // (frame * tiles + tile) * 64
        const int pred = tile > 0 ? meta_dc(sp.meta[u0 - 64 + 63]) : 0;
        const int dc = meta_dc(sp.meta[u0]);
        uint32_t len = 0;
        auto count = [&](uint32_t, uint32_t l) { len += l; };
        if (!put_dc(dc - pred, s_dcl, count)) atomicOr(sp.status, 1u), POISON_FT();  // MI355_E_CATEGORY
        atomicAdd(&sp.tile_bits[ft], len);
    }
}

// ----------------------------------------------------------------------------
// DC predictor of a unit from `meta`: the previous lane, or the last block of the previous tile (P passes per tile).
// ----------------------------------------------------------------------------
template <uint32_t P = 3>
__device__ __forceinline__ int meta_pred(const uint32_t* __restrict__ meta, uint32_t frame_tile0, uint32_t tile,
                                         uint32_t chan, uint32_t lane, int own_dc) {
    int prev = __shfl_up(own_dc, 1);
    if (lane == 0) {
        prev = 0;
        if (tile > 0) prev = meta_dc(meta[((frame_tile0 + tile - 1) * P + chan) * 64 + 63]);
    }
    return prev;
}

// ----------------------------------------------------------------------------
// k_merge: like k_emit, but the AC bits come ready-made from the arena.
// ----------------------------------------------------------------------------
// S420: the tile is 64 MCUs = 384 units; thread t = 6 * mcu + k is the unit at position t of the
// tile's scan (k < 4: luma block k of the MCU = unit 4 mcu + k of the tile's 256 luma units, which the
// encode kernel stored as pass (4 mcu + k) / 64, lane (4 mcu + k) % 64; k = 4, 5: Cb, Cr).
// Launch bounds of 256 for the 192-thread form on purpose: for a three-wave workgroup with this much LDS the compiler
// works out that at most seven waves fit a SIMD and then RAISES the kernel's register allocation to the most seven waves
// allow -- 72 instead of the 32 it uses (.amdhsa_next_free_vgpr 65) -- and with 72 a k_merge wave only fits beside two
// k_screen_encode waves of at most 216 registers (found in round 4 when the encode kernel went to 221 and batched calls
// lost a quarter; tests/test_kernel_budget.py reads the allocation from the kernel descriptors now).
// SMALL: the bit-assembly window at half size (kEmitLdsWordsSmall), so that TWO workgroups of this kernel fit a CU beside
// two of k_screen_encode: batches run this form.  With one workgroup per CU the merge of a part takes about as long as
// the block encode it runs beside, and whenever it takes longer -- parts of unequal size, say 124 frames per call -- its
// workgroups are still streaming through the CUs when the NEXT launch's persistent workgroups arrive: a CU that holds
// two of them has no room for its second encode workgroup (72 KB of LDS), and that workgroup stays out until the
// following k_merge is through as well (rocprofv3 timeline, gpurun r4tl: launches of 540-830 us instead of 500; 232
// instead of 256 Gpixel/s at 100, 124, 132 frames per call).  At two per CU the merge is done well before the launch it
// runs beside (gpurun r4w2: 256 Gpixel/s at every batch size tried).  Tiles beyond 64 000 bits (15.6 bit per pixel)
// assemble their bits in device memory instead.
template <bool S420, bool SMALL>
__global__ void __launch_bounds__(S420 ? 384 : 256)
    k_merge(Geom g, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ pass_off, const uint32_t* __restrict__ arena,
            const uint32_t* __restrict__ lut, const uint64_t* __restrict__ tile_off,
            uint8_t* __restrict__ out, uint64_t out_stride, const uint64_t* __restrict__ frame_bits,
            uint32_t lds_words_limit) {
    constexpr bool GRAY = false;
#include "jpeg_merge_body.h"
}

// Gray: one component, one unit per scan step -- a 64-thread workgroup (one wave) per tile of 64 units.  The half-window
// form is what batched calls run: two of its workgroups per CU fit beside two of k_gray_encode like k_merge's do beside
// k_screen_encode (tests/test_gray_kernel_budget.py).  Launch bounds of 256 for the 64-thread form for the reason given
// above k_merge: with 64 the compiler works out an occupancy from the LDS alone and raises the allocation to what it
// allows (88 registers for the half window, 136 for the full one, 27 used), which no longer fits beside the encode.
template <bool SMALL>
__global__ void __launch_bounds__(256)
    k_gray_merge(Geom g, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ pass_off, const uint32_t* __restrict__ arena,
                 const uint32_t* __restrict__ lut, const uint64_t* __restrict__ tile_off,
                 uint8_t* __restrict__ out, uint64_t out_stride, const uint64_t* __restrict__ frame_bits,
                 uint32_t lds_words_limit) {
    constexpr bool S420 = false, GRAY = true;
#include "jpeg_merge_body.h"
}

// ----------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------
// Number of persistent WAVES (4 per workgroup).  Full groups of 8 workgroups whenever the
// work allows, so that the XCD-aware tile mapping applies.
uint32_t screen_grid(const Geom& g, uint32_t n_frames, uint32_t max_waves) {
    uint32_t total = g.tiles * g.passes * n_frames;
    uint32_t wgs = (total + kEncWaves - 1) / kEncWaves;
    uint32_t max_wgs = max_waves / kEncWaves ? max_waves / kEncWaves : 1;
    if (wgs > max_wgs) wgs = max_wgs;
    if (wgs >= 8) wgs &= ~7u;
    return wgs * kEncWaves;
}
hipError_t launch_screen_encode(const Geom& g, uint32_t n_frames, const uint8_t* rgb, const ScreenParams& sp,
                                bool probe, uint32_t grid_waves, hipStream_t s) {
    uint32_t grid = screen_grid(g, n_frames, grid_waves) / kEncWaves;
    const int mode = is420(g) ? 2 : ((g.flags & 2u) ? 1 : 0);  // MI355_F_STANDARD, 4:2:0
#define MI355_LAUNCH_ENC(PR, MD) \
    hipLaunchKernelGGL((k_screen_encode<PR, MD>), dim3(grid), dim3(256), 0, s, g, n_frames, rgb, sp)
    if (is_gray(g)) {
        if (probe) hipLaunchKernelGGL((k_gray_encode<true>), dim3(grid), dim3(256), 0, s, g, n_frames, rgb, sp);
        else hipLaunchKernelGGL((k_gray_encode<false>), dim3(grid), dim3(256), 0, s, g, n_frames, rgb, sp);
    } else if (probe) {
        if (mode == 2) MI355_LAUNCH_ENC(true, 2);
        else if (mode == 1) MI355_LAUNCH_ENC(true, 1);
        else MI355_LAUNCH_ENC(true, 0);
    } else {
        if (mode == 2) MI355_LAUNCH_ENC(false, 2);
        else if (mode == 1) MI355_LAUNCH_ENC(false, 1);
        else MI355_LAUNCH_ENC(false, 0);
    }
#undef MI355_LAUNCH_ENC
    return hipGetLastError();
}
hipError_t launch_dc_heads(const Geom& g, uint32_t n_frames, const ScreenParams& sp, hipStream_t s) {
    // one lane per (tile, pass) head when the batch is small, a few per lane when it is large
    const uint64_t heads = (uint64_t)n_frames * g.tiles * g.passes;
    const uint32_t head_waves = (uint32_t)((heads + 63) / 64 < 4096 ? (heads + 63) / 64 : 4096);
    if (is_gray(g)) hipLaunchKernelGGL(k_gray_dc_heads, dim3(head_waves), dim3(64), 0, s, g, n_frames, sp);
    else hipLaunchKernelGGL(k_dc_heads, dim3(head_waves), dim3(64), 0, s, g, n_frames, sp);
    return hipGetLastError();
}
hipError_t launch_merge(const Geom& g, uint32_t n_frames, const uint32_t* meta, const uint32_t* pass_off, const uint32_t* arena,
                        const uint32_t* lut, const uint64_t* tile_off,
                        uint8_t* out, uint64_t out_stride, const uint64_t* frame_bits, uint32_t lds_words_limit,
                        bool small_window, hipStream_t s) {
    if (lds_words_limit > kEmitLdsWords) lds_words_limit = kEmitLdsWords;
#define MI355_LAUNCH_MERGE(S4, SM, NT) \
    hipLaunchKernelGGL((k_merge<S4, SM>), dim3(g.tiles, n_frames), dim3(NT), 0, s, g, meta, pass_off, arena, lut, tile_off, out, \
                       out_stride, frame_bits, lds_words_limit)
    if (is_gray(g)) {
        if (small_window)
            hipLaunchKernelGGL((k_gray_merge<true>), dim3(g.tiles, n_frames), dim3(64), 0, s, g, meta, pass_off, arena, lut,
                               tile_off, out, out_stride, frame_bits, lds_words_limit);
        else
            hipLaunchKernelGGL((k_gray_merge<false>), dim3(g.tiles, n_frames), dim3(64), 0, s, g, meta, pass_off, arena, lut,
                               tile_off, out, out_stride, frame_bits, lds_words_limit);
    } else if (is420(g)) {
        if (small_window) MI355_LAUNCH_MERGE(true, true, 384);
        else MI355_LAUNCH_MERGE(true, false, 384);
    } else {
        if (small_window) MI355_LAUNCH_MERGE(false, true, 192);
        else MI355_LAUNCH_MERGE(false, false, 192);
    }
#undef MI355_LAUNCH_MERGE
    return hipGetLastError();
}

}  // namespace mi355
