// mfma_h_common.hpp -- the one home of what the matrix-core scans share (K1e hamming_mfma.hip, K1f hamming_mfma_g.hip,
// K1g hamming_mfma_d.hip, K1h hamming_mfma_h.hip, K1i hamming_mfma_i.hip), and of the key / popcount helpers the XOR + popcount
// scans (hamming.hip) and the stages behind a scan (match_post.hip) share with them.  Two parts: (1) what every scan uses --
// vector and address-space typedefs, fp4 operand codes, packed 16-bit key operations, the raw-row Hamming distance; (2) the
// MH_* layout constants of K1h / K1i (and of their merge) alone.
// Every helper is __forceinline__ and carries the one comment that says why it is written as it is.
// Internal to libplslam_hip.so.
#pragma once

#include "match_kernels.hpp"   // the launch interface of the scans and of the stages behind them (+ common.hpp)

namespace plslam {
// ---- part 1: every matrix-core scan ---------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4), aligned(4)));   // descriptor rows are only 4-byte aligned
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
// Pointers read from the launch tables are GENERIC to the compiler, and a generic access is a FLAT instruction, which
// counts on lgkmcnt as well as vmcnt: the `s_waitcnt lgkmcnt(0)` in front of every workgroup barrier then waits for
// the raw-row PREFETCH of two tiles ahead (round 2 finding: every tile paid a memory latency).  With the address
// space spelled out the loads are global_load (vmcnt only) and stay in flight across the barrier.
#define PLSLAM_GLOBAL __attribute__((address_space(1)))
typedef const PLSLAM_GLOBAL uint32_t* gcu32_t;
typedef const PLSLAM_GLOBAL u32x4_t* gcu32x4_t;
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef PLSLAM_GLOBAL u32x2_t* gu2_t;
typedef const PLSLAM_GLOBAL u32x2_t* gu2c_t;
typedef PLSLAM_GLOBAL uint32_t* gu32_t;

namespace {

// fp4 (e2m1) codes: +1.0 = 0x2, -1.0 = 0xA.  b side: bit 0 -> +1, bit 1 -> -1 = s(b); the a side is the b code
// XOR 0x8 per nibble (= -s(a)) and carries the block scale 2^6 (E8M0 133), the b side 2^0 (E8M0 127).
constexpr uint32_t FP4_NEG = 0x88888888u;
constexpr uint32_t FP4_ONE = 0x22222222u;
constexpr uint32_t FP4_FOUR = 0x66666666u;    // e2m1 code 0b0110 = 4.0
constexpr int SCALE_A = 133, SCALE_B = 127;
constexpr uint32_t ACC_BITS = 0x4B000000u + 16384u;   // float bits of 2^23 + 16384 (+ small integers: + the integer)
// 16-bit keys are (d << 7) | tag7: the A codes are -64 s(a), so with C = 16384 + tag the accumulator
// itself is 128 d + tag (<= (256 << 7) + 127 = 0x807F); anything above is "none"
constexpr uint32_t KEY16_MAX = 0x807Fu;

__device__ __forceinline__ uint32_t umin_(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax_(uint32_t a, uint32_t b) { return a > b ? a : b; }
// merge two sorted pairs of keys
__device__ __forceinline__ void merge2(uint32_t& a0, uint32_t& a1, uint32_t c0, uint32_t c1)
{
    const uint32_t lo = umin_(a0, c0);
    const uint32_t hi = umin_(umax_(a0, c0), umin_(a1, c1));
    a0 = lo;
    a1 = hi;
}
// packed 16-bit min / max / saturating add.  Inline asm on purpose: written with the vector builtins the compiler sinks
// the row-direction pushes out of the MFMA block into a block of their own (K1e: 96 VALU ops with no MFMA to
// hide under, 6 spilled VGPRs; measured 6.10 ms vs 5.85 ms).  They only ever see pack_acc's result, never an accumulator.
__device__ __forceinline__ uint32_t pk_min16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_max16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_add16_sat(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_add_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// two sorted streams of 16-bit keys, one per half of the register
__device__ __forceinline__ void pk_push2(uint32_t& b0, uint32_t& b1, uint32_t key)
{
    b1 = pk_min16(b1, pk_max16(b0, key));
    b0 = pk_min16(b0, key);
}
// accumulators of the two M-tiles (2^23 + 128 d + tag, tag <= 127) side by side: hi.lo16 << 16 | lo.lo16.
// The BUILTIN, never inline asm: this is the one instruction that reads MFMA results directly, and on gfx950 the
// wait states between an MFMA and a VALU access to its destination registers are the COMPILER's job (s_nop); its
// hazard recognizer does not look inside asm statements.  As `asm("v_perm_b32 ...")` the first two packs of K1e's
// unpipelined epilogue issued right behind the last MFMA of the set: accumulators 0 and 1 (tile rows 0, 1, 4, 5)
// were read -- and register 0 overwritten -- while still in flight.  Right most of the time, wrong when waves of
// co-resident workgroups delayed the matrix pipe: ~1 % of the intermediate keys of a loaded batch differed from
// run to run, 1e-6 of the table entries at a 0.9 ratio ("K1e determinism";
// tools/determinism_check.py is the instrument).
__device__ __forceinline__ uint32_t pack_acc(float lo, float hi)
{
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi), __builtin_bit_cast(uint32_t, lo), 0x05040100u);
}
__device__ __forceinline__ uint32_t key16_to_key32(uint32_t k16, uint32_t tag_bias, uint32_t idx_base,
                                                   uint32_t idx_scale)
{
    return k16 > KEY16_MAX ? KEY_NONE
                           : (((k16 >> 7) << KEY_IDX_BITS) | (idx_base + ((k16 & 127u) - tag_bias) * idx_scale));
}
// 32 bits of a descriptor -> 32 fp4 codes of s(bit): dword s holds bits 4k + s, nibble k = MAG | bit << 3.
// MAG: the magnitude code in every nibble (FP4_ONE = 1.0; K1i's unscaled form: FP4_FOUR = 4.0).
// 7 VALU ops of the fast class (measured ~2.5 cycles per wave instruction against ~4.2 for shifts and v_and_or): three adds
// for x << 1, 2, 3 and four v_bitop3 (a & b) | c.  Written with asm / the builtin because the compiler turns x + x back
// into a shift and (x & m) | c into v_and + v_or.
template <bool A_SIDE, uint32_t MAG = FP4_ONE>
__device__ __forceinline__ i32x4 expand_dword_fp4(uint32_t x)
{
    uint32_t x1, x2, x3;
    asm("v_add_u32 %0, %1, %1" : "=v"(x1) : "v"(x));
    asm("v_add_u32 %0, %1, %1" : "=v"(x2) : "v"(x1));
    asm("v_add_u32 %0, %1, %1" : "=v"(x3) : "v"(x2));
    constexpr uint32_t base = A_SIDE ? (MAG ^ FP4_NEG) : MAG;               // a side: sign nibble-bit flipped
    constexpr unsigned TT = A_SIDE ? 0x6Au : 0xEAu;                         // (a & b) ^ c  |  (a & b) | c
    i32x4 v;
    v.x = (int)__builtin_amdgcn_bitop3_b32(x3, FP4_NEG, base, TT);
    v.y = (int)__builtin_amdgcn_bitop3_b32(x2, FP4_NEG, base, TT);
    v.z = (int)__builtin_amdgcn_bitop3_b32(x1, FP4_NEG, base, TT);
    v.w = (int)__builtin_amdgcn_bitop3_b32(x, FP4_NEG, base, TT);
    return v;
}
// r = popcount(x) + acc in ONE VALU op (asm: the compiler would otherwise re-associate the chain)
__device__ __forceinline__ uint32_t bcnt_acc_(uint32_t x, uint32_t acc)
{
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
// the raw-row distance of the second-best recomputation: 8 XOR + 8 accumulating popcounts
__device__ __forceinline__ uint32_t hamming256(u32x4_t a_lo, u32x4_t a_hi, u32x4_t b_lo, u32x4_t b_hi)
{
    uint32_t d = bcnt_acc_(a_lo.x ^ b_lo.x, 0u);
    d = bcnt_acc_(a_lo.y ^ b_lo.y, d);
    d = bcnt_acc_(a_lo.z ^ b_lo.z, d);
    d = bcnt_acc_(a_lo.w ^ b_lo.w, d);
    d = bcnt_acc_(a_hi.x ^ b_hi.x, d);
    d = bcnt_acc_(a_hi.y ^ b_hi.y, d);
    d = bcnt_acc_(a_hi.z ^ b_hi.z, d);
    d = bcnt_acc_(a_hi.w ^ b_hi.w, d);
    return d;
}
// XCD-striped block tables: hardware places workgroup b on XCD b % 8 and dispatches in increasing
// b; the host lays the table out as 8 rows of L = gridDim.x / 8 entries, row x = the work of XCD x in
// dispatch order (match_planner.hpp, deal_to_xcds), so the blocks of one problem -- which stream the same
// descriptor sets -- sit on one XCD's L2 at the same time.  Rows are padded with item = -1.
__device__ __forceinline__ int xcd_remap_(int orig, int nwg) { return (orig & 7) * (nwg >> 3) + (orig >> 3); }

// ---- part 2: the layouts of K1h / K1i alone --------------------------------------------------------------------------------
constexpr int MH_TILE_N = 32;                 // b rows per tile
constexpr int MH_KSTEPS = 4;                  // 256 bits = 4 x K 64
constexpr int MH_ROW_STRIDE = 144;            // bytes per expanded b row in LDS (128 + 16: 4-bank skew)
constexpr int MH_TILE_BYTES = MH_TILE_N * MH_ROW_STRIDE;
constexpr int MH_GROUP = 16;                  // tiles per group of the row direction (512 b rows)
constexpr int MH_GROUP_ROWS = MH_GROUP * MH_TILE_N;
constexpr int MH_WINDOW = 64;                 // tiles per window: the row keys' tag holds the group within the window (2 bits)
constexpr int MH_MERGE_SPT = 4;               // slots per lane of the merge kernel (PARTS == 1)
// (round 5) the one-word-per-entry merge requests the words of up to this many row blocks together -- a 1500-row problem's
// six in ONE round trip instead of three
constexpr int MH_MERGE_WB = 8;
constexpr int MH_CGROUP = 8;                  // tiles whose column results are staged in LDS and stored together (256 slots)
// a column that does not exist: zero codes (the contraction contributes nothing: "distance 128") + this in the seed
// = key 0xBF80 + tag: above KEY16_MAX, below the 16-bit wrap
constexpr uint32_t COL_PENALTY = 0x7F80u;

}  // namespace

}  // namespace plslam
