// inflate_tables.h -- device code shared by the two inflate kernels (csrc/inflate.hip: one wavefront per BGZF member;
// csrc/gzip_stream.hip: one wavefront per chunk of a plain gzip stream): the wave's prefix sum, the entries of the Huffman
// tables, the tables built by the wave in parallel, and canonical decoding of the codes longer than a table's index bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

template <int CTRL, int RMASK>
__device__ __forceinline__ int dpp_add(int x) { return x + __builtin_amdgcn_update_dpp(0, x, CTRL, RMASK, 0xf, false); }
// inclusive sum over the 64 lanes: four row_shr steps, then row_bcast15 / row_bcast31
__device__ __forceinline__ int wave_scan_add(int x) {
  x = dpp_add<0x111, 0xf>(x);
  x = dpp_add<0x112, 0xf>(x);
  x = dpp_add<0x114, 0xf>(x);
  x = dpp_add<0x118, 0xf>(x);
  x = dpp_add<0x142, 0xa>(x);
  x = dpp_add<0x143, 0xc>(x);
  return x;
}

// ---- table entries: everything a lane needs to know about a code, so that decoding is two lookups and a few shifts
// literal / length code:  bits 0-3 code length (0: no code this short starts with these bits), 4-5 kind (0 literal, 1 length,
//   2 end of block, 3 none / invalid), 6-8 number of extra bits, 9-17 the literal or the length's base
constexpr uint32_t LIT_NONE = 3u << 4;
struct LitEntry {
 __device__ __forceinline__ uint32_t operator()(uint32_t s, uint32_t ml) const {
  if (s < 256u) return ml | (s << 9);
  if (s == 256u) return ml | (2u << 4);
  if (s > 285u) return ml | (3u << 4);
  const uint32_t ls = s - 257u;
  const uint32_t lx = ls < 8u || ls == 28u ? 0u : (ls >> 2) - 1u;
  const uint32_t lb = ls < 8u ? 3u + ls : ls == 28u ? 258u : 3u + ((4u + (ls & 3u)) << lx);
  return ml | (1u << 4) | (lx << 6) | (lb << 9);
 }
};
// distance code: bits 0-3 code length (0: none), 4-7 number of extra bits, 8-23 base
struct DstEntry {
 __device__ __forceinline__ uint32_t operator()(uint32_t s, uint32_t ml) const {
  if (s > 29u) return 0u;
  const uint32_t dx = s < 4u ? 0u : (s >> 1) - 1u;
  const uint32_t db = s < 4u ? 1u + s : 1u + ((2u + (s & 1u)) << dx);
  return ml | (dx << 4) | (db << 8);
 }
};
struct LenEntry {
  __device__ __forceinline__ uint16_t operator()(uint32_t s, uint32_t ml) const { return (uint16_t)((s << 4) | ml); }
};

// Canonical Huffman code of n symbols with lengths lens[0..n): table of 2^tb entries (make(symbol, length); `none` where a
// longer code or none starts), per-length counts and the symbols sorted by (length, symbol) for the bit-by-bit decoder.
// Returns false if the lengths over-subscribe the code space.
template <class T, class F>
__device__ bool build_table(const uint8_t* lens, int n, T* tab, int tb, uint16_t* cnt, uint16_t* sym, int lane, T none, F make,
                            uint32_t* state = nullptr) {   // the bit-by-bit decoder's first << 16 | index after tb levels
  for (int k = lane; k < (1 << tb); k += 64) tab[k] = none;
  int count[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int s = s0 + lane;
    const int ml = s < n ? (int)lens[s] : 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) count[l] += (int)__popcll(__ballot(ml == l));
  }
  int offs[16], code0[16];
  int left = 1, code = 0, o = 0;
  offs[0] = 0; code0[0] = 0;
  bool over = false;
#pragma unroll
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - count[l];
    if (left < 0) over = true;
    code = (code + (l > 1 ? count[l - 1] : 0)) << 1;
    code0[l] = code;
    offs[l] = o;
    o += count[l];
  }
  if (over) return false;
  if (state) {
    int f = 0, ix = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l)
      if (l <= tb) { ix += count[l]; f = (f + count[l]) << 1; }
    *state = ((uint32_t)f << 16) | (uint32_t)ix;
  }
  if (lane < 16) {
    int c = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) c = lane == l ? count[l] : c;
    cnt[lane] = (uint16_t)c;
  }
  int run[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) run[l] = 0;
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int s = s0 + lane;
    const int ml = s < n ? (int)lens[s] : 0;
    int rank = 0, first = 0, base = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
      const unsigned long long m = __ballot(ml == l);
      if (ml == l) { rank = run[l] + (int)__popcll(m & lt); first = code0[l]; base = offs[l]; }
      run[l] += (int)__popcll(m);
    }
    if (ml) {
      sym[base + rank] = (uint16_t)s;
      if (ml <= tb) {
        const uint32_t rev = __brev((uint32_t)(first + rank)) >> (32 - ml);
        const T e = make((uint32_t)s, (uint32_t)ml);
        for (uint32_t k = rev; k < (1u << tb); k += (1u << ml)) tab[k] = e;
      }
    }
  }
  return true;
}

// A code longer than the direct table's tb index bits, decoded canonically from level tb + 1 on by the lane that met it:
// bits = the stream from the code's first bit (at least 15 valid), state = the decoder's first << 16 | index after tb
// levels.  Symbol | length << 16, or ~0 when no code of at most 15 bits starts like this.
__device__ __forceinline__ uint32_t long_code(uint32_t bits, int tb, uint32_t state, const uint16_t* cnt, const uint16_t* sym) {
  int code = (int)(__brev(bits) >> (32 - tb)) << 1, first = (int)(state >> 16), index = (int)(state & 0xffffu);
  uint32_t b = bits >> tb;
  for (int l = tb + 1; l <= 15; ++l) {
    code |= (int)(b & 1u);
    b >>= 1;
    const int count = (int)cnt[l];
    if (code - count < first) return (uint32_t)sym[index + (code - first)] | ((uint32_t)l << 16);
    index += count; first += count; first <<= 1; code <<= 1;
  }
  return ~0u;
}

}  // namespace
