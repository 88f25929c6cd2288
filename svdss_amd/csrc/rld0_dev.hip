// rld0_dev.hip -- the rld0 (`.fmd`) ENCODER on the device: the file rld0_write (rld0.cpp) writes, byte for byte, from the
// rank blocks in HBM.  The rule the format imposes is rld0_plan.h; the stages:
//
//   planes   run starts straight from the bit planes of the rank blocks (each plane XOR itself shifted by one symbol, the
//            carry taken from the quarter before), counted per quarter, scanned, compacted as int64 with their symbols
//   plan     code widths and their prefix sums
//   chain    per tile of runs a table entry state -> exit state + block count (a lane per entry state, no block numbers);
//            ONE lane walks the tables in order and carries the block number (a tile a piece ends in is walked block by
//            block); every tile then re-walks from its true entry and writes block descriptors
//   emit     a lane per block: header from the descriptor before it, codes, 64 bytes
//   download the data words in slices through two page-locked buffers while the slice before is written and its headers
//            go into the rank frames; the writer never seeks
//
// The device declines whole calls (the host encoder writes the file then): n == 0, a block of SVDSS_FMD_DECLINE_SYMS
// (2^30) symbols or more, a plan that does not fit in free HBM, no GPU / SVDSS_INDEX_CPU.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/svdss_hip.h"
#include "fmd_layout.h"
#include "hip_check.h"
#include "index_host.h"
#include "rld0.h"
#include "rld0_plan.h"

namespace {

constexpr int ENTRY_STATES = RLD0_ENTRY_STATES;
constexpr int64_t SCAN_CHUNK_MAX = (int64_t)1 << 30;    // hipcub counts its items in an int

struct Last { int32_t route = -1; int64_t runs = 0, blocks = 0, pieces = 0; double ms[6] = {0, 0, 0, 0, 0, 0}; };
thread_local Last g_last;

// bit i: symbol 32 q + i starts a run.  (p1 of '$' / N is masked: the layout says 0, an old file may not)
__device__ uint32_t run_start_mask(const svdss_u4* bl, int64_t q, int64_t n, uint32_t* p0, uint32_t* p1, uint32_t* p2) {
  const svdss_u4 a = bl[q];
  *p0 = a.y; *p2 = a.w; *p1 = a.z & ~a.w;
  uint32_t c0 = 0, c1 = 0, c2 = 0;
  if (q > 0) {
    const svdss_u4 b = bl[q - 1];
    c0 = b.y >> 31; c1 = (b.z & ~b.w) >> 31; c2 = b.w >> 31;
  }
  uint32_t m = (*p0 ^ (*p0 << 1 | c0)) | (*p1 ^ (*p1 << 1 | c1)) | (*p2 ^ (*p2 << 1 | c2));
  if (q == 0) m |= 1u;
  const int64_t valid = n - 32 * q;
  return m & svdss_lowmask(valid > 32 ? 32 : valid < 0 ? 0 : (int)valid);
}

// Every kernel below walks its items in a grid-stride loop: a grid is at most GRID_MAX workgroups (a launch of 2^32
// work-items or more -- the runs of a human genome's BWT -- wraps without an error), SVDSS_FMD_GRID_BLOCKS for the tests.
#define FOR_EACH_ITEM(i, count) \
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (count); i += (int64_t)gridDim.x * 256)

// cnt[q + 1] = run starts in quarter q, cnt[0] = 0: the inclusive scan of cnt is the first run of every quarter
__global__ void __launch_bounds__(256) k_count(const svdss_u4* bl, int64_t n, int64_t nq, int64_t* cnt) {
  FOR_EACH_ITEM(q, nq) {
    uint32_t p0, p1, p2;
    cnt[q + 1] = __popc(run_start_mask(bl, q, n, &p0, &p1, &p2));
    if (q == 0) cnt[0] = 0;
  }
}

__global__ void __launch_bounds__(256) k_scatter(const svdss_u4* bl, int64_t n, int64_t nq, const int64_t* first, int64_t R,
                                                 int64_t* start, uint8_t* sym) {
  FOR_EACH_ITEM(q, nq) {
    uint32_t p0, p1, p2;
    uint32_t m = run_start_mask(bl, q, n, &p0, &p1, &p2);
    int64_t at = first[q];
    while (m) {
      const int bit = __ffs(m) - 1;
      m &= m - 1;
      if (at < R) {
        const uint32_t b0 = (p0 >> bit) & 1u, b1 = (p1 >> bit) & 1u, b2 = (p2 >> bit) & 1u;
        start[at] = 32 * q + bit;
        sym[at] = (uint8_t)(b2 ? (b0 ? 5 : 0) : 1u + (b1 << 1 | b0));
      }
      ++at;
    }
    if (q == 0) start[R] = n;
  }
}

// W[r + 1] = bits of run r's code, W[0] = 0: the inclusive scan of W is the exclusive prefix sum P
__global__ void __launch_bounds__(256) k_width(const int64_t* start, int64_t R, int64_t* W) {
  FOR_EACH_ITEM(r, R) {
    W[r + 1] = rld0_code_width(start[r + 1] - start[r]);
    if (r == 0) W[0] = 0;
  }
}

__global__ void k_carry(int64_t* a) { a[0] += a[-1]; }

// the chain's stages (rld0_plan.h), a lane per table entry / one lane / a lane per tile / a lane per block
__global__ void __launch_bounds__(256) k_tables(const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t n_tiles, uint32_t* table) {
  FOR_EACH_ITEM(g, n_tiles * ENTRY_STATES) table[g] = rld0_table_entry(start, P, R, T, g / ENTRY_STATES, (int)(g % ENTRY_STATES));
}

__global__ void k_walker(const uint32_t* table, const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t n_tiles,
                         int64_t piece_words, uint32_t* entry_state, int64_t* entry_block, int64_t* res) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  rld0_walk_tables(table, start, P, R, T, n_tiles, piece_words, entry_state, entry_block, res);
}

__global__ void __launch_bounds__(256) k_desc(const int64_t* start, const int64_t* P, int64_t R, int64_t T, int64_t n_tiles, int64_t piece_words,
                                              const uint32_t* entry_state, const int64_t* entry_block, int64_t B, int64_t decline_syms,
                                              int64_t* desc, int32_t* flag) {
  FOR_EACH_ITEM(t, n_tiles) {
    const int got = rld0_tile_desc(start, P, R, T, n_tiles, piece_words, t, entry_state, entry_block, B, decline_syms, desc);
    if (got & 1) flag[0] = 1;
    if (got & 2) flag[1] = 1;
  }
}

__global__ void __launch_bounds__(256) k_emit(const int64_t* start, const uint8_t* sym, int64_t R, const int64_t* desc, int64_t B, uint64_t* out) {
  FOR_EACH_ITEM(b, B + 1) rld0_emit_desc(start, sym, R, desc, B, b, out);
}

int64_t env_i64(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return e && *e ? atoll(e) : dflt;
}

// a[0, count) summed inclusively in place, in chunks hipcub can count: 2^30 items, SVDSS_FMD_SCAN_ITEMS for the tests (the
// runs of a human genome's BWT take five chunks; k_carry hands the total so far to the next one)
int scan_in_place(int64_t* a, int64_t count) {
  const int64_t SCAN_CHUNK = std::max<int64_t>(2, std::min(env_i64("SVDSS_FMD_SCAN_ITEMS", SCAN_CHUNK_MAX), SCAN_CHUNK_MAX));
  void* tmp = nullptr;
  size_t tb = 0;
  const int first = (int)std::min(count, SCAN_CHUNK);
  HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, a, a, first, 0));
  HIPCHK(hipMalloc(&tmp, tb ? tb : 16));
  int rc = SVDSS_OK;
  for (int64_t at = 0; at < count && rc == SVDSS_OK; at += SCAN_CHUNK) {
    const int m = (int)std::min(SCAN_CHUNK, count - at);
    if (at > 0) hipLaunchKernelGGL(k_carry, dim3(1), dim3(1), 0, 0, a + at);
    size_t tb2 = tb;
    if (hipcub::DeviceScan::InclusiveSum(tmp, tb2, a + at, a + at, m, 0) != hipSuccess) rc = SVDSS_EHIP;
  }
  if (hipDeviceSynchronize() != hipSuccess) rc = SVDSS_EHIP;
  (void)hipFree(tmp);
  return rc;
}

double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

struct Bufs {   // freed however the call ends; alloc_ms: what hipMalloc / hipFree took, inside the stages' timers (SVDSS_DEBUG prints it)
  std::vector<void*> dev, pinned;
  double alloc_ms = 0;
  template <class T> hipError_t get(T** p, size_t bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipMalloc((void**)p, bytes ? bytes : 16);
    alloc_ms += since(t0);
    if (e == hipSuccess) dev.push_back((void*)*p);
    return e;
  }
  void drop(void* p) { const auto t0 = std::chrono::steady_clock::now(); (void)hipFree(p); alloc_ms += since(t0); dev.erase(std::find(dev.begin(), dev.end(), p)); }
  ~Bufs() { for (void* p : dev) (void)hipFree(p); for (void* p : pinned) (void)hipHostFree(p); }
};

// does an allocation of `need` bytes leave 64 MB of the free HBM?  SVDSS_FMD_HBM_LIMIT_MB (a test knob): as if no more than
// that were free.  Another thread may allocate between the question and the allocation (the sidecar's thread fetches the
// text): an allocation that then fails for lack of memory declines the call as well (rld0_dev_encode).
bool fits(size_t need) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const int64_t limit_mb = env_i64("SVDSS_FMD_HBM_LIMIT_MB", -1);
  if (limit_mb >= 0) free_b = std::min(free_b, (size_t)limit_mb << 20);
  return need + ((size_t)64 << 20) <= free_b;
}

constexpr int64_t GRID_MAX = (int64_t)1 << 22;   // workgroups of 256: 2^30 work-items a launch at most
inline unsigned grid_for(int64_t items) {
  int64_t cap = env_i64("SVDSS_FMD_GRID_BLOCKS", GRID_MAX);
  cap = std::max<int64_t>(1, std::min(cap, GRID_MAX));
  return (unsigned)std::max<int64_t>(1, std::min((items + 255) / 256, cap));
}

}  // namespace

void rld0_encode_note(int32_t route, double total_ms) {
  g_last = Last();
  g_last.route = route;
  g_last.ms[5] = total_ms;
}

static int encode_on_device(const void* d_blocks_v, int64_t n, const int64_t acc[7], const char* path);

// The `.fmd` of the BWT behind the rank blocks d_blocks (resident on the current device) -> path.  SVDSS_OK: written on the
// device; a negative value -(route): declined, nothing written (2 = empty, 3 = block total, 4 = memory); else an error.
// (Every allocation, the page-locked buffers included, comes before the file is opened: one that fails for lack of memory
// -- the question to hipMemGetInfo is not a reservation -- declines the call like a plan that does not fit.)
int rld0_dev_encode(const void* d_blocks_v, int64_t n, const int64_t acc[7], const char* path) {
  const int rc = encode_on_device(d_blocks_v, n, acc, path);
  if (rc == SVDSS_ENOMEM) { (void)hipGetLastError(); return -SVDSS_FMD_DECLINED_MEMORY; }
  return rc;
}

static int encode_on_device(const void* d_blocks_v, int64_t n, const int64_t acc[7], const char* path) {
  const svdss_u4* d_blocks = (const svdss_u4*)d_blocks_v;
  if (n <= 0) return -SVDSS_FMD_DECLINED_EMPTY;
  const auto t_all = std::chrono::steady_clock::now();
  Last L;
  int64_t T = env_i64("SVDSS_FMD_TILE_RUNS", 4096);
  T = std::max<int64_t>(RLD0_MAX_BLOCK_RUNS, std::min<int64_t>(T, 65536));
  int64_t decline_syms = env_i64("SVDSS_FMD_DECLINE_SYMS", RLD0_TYPE2_SYMS);
  decline_syms = std::max<int64_t>(1, std::min<int64_t>(decline_syms, RLD0_TYPE2_SYMS));
  const int64_t piece_words = RLD0_PIECE_WORDS;
  Bufs B_;
  // ---- planes
  auto t0 = std::chrono::steady_clock::now();
  const int64_t nq = 4 * (n / SVDSS_BLOCK_SYMS + 1);
  if (!fits((size_t)(nq + 1) * 8)) return -SVDSS_FMD_DECLINED_MEMORY;
  int64_t* d_first = nullptr;
  HIPCHK(B_.get(&d_first, (size_t)(nq + 1) * 8));
  hipLaunchKernelGGL(k_count, dim3(grid_for(nq)), dim3(256), 0, 0, d_blocks, n, nq, d_first);
  HIPCHK(hipGetLastError());
  { const int rc = scan_in_place(d_first, nq + 1); if (rc != SVDSS_OK) return rc; }
  int64_t R = 0;
  HIPCHK(hipMemcpy(&R, d_first + nq, 8, hipMemcpyDeviceToHost));
  if (R <= 0 || R > n) { g_svdss_hip_err = "rld0 device encoder: run count out of range"; return SVDSS_EHIP; }
  const int64_t n_tiles = (R + T - 1) / T;
  // 17 bytes per run (start 8, prefix sum 8, symbol 1), 780 per tile (192 table entries of 4, entry state 4, entry block 8)
  if (!fits((size_t)(R + 1) * 17 + (size_t)n_tiles * (ENTRY_STATES * 4 + 12))) return -SVDSS_FMD_DECLINED_MEMORY;
  int64_t *d_start = nullptr, *d_P = nullptr;
  uint8_t* d_sym = nullptr;
  HIPCHK(B_.get(&d_start, (size_t)(R + 1) * 8));
  HIPCHK(B_.get(&d_sym, (size_t)(R + 1)));
  hipLaunchKernelGGL(k_scatter, dim3(grid_for(nq)), dim3(256), 0, 0, d_blocks, n, nq, d_first, R, d_start, d_sym);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  B_.drop(d_first);
  L.ms[0] = since(t0);
  // ---- plan
  t0 = std::chrono::steady_clock::now();
  HIPCHK(B_.get(&d_P, (size_t)(R + 1) * 8));
  hipLaunchKernelGGL(k_width, dim3(grid_for(R)), dim3(256), 0, 0, d_start, R, d_P);
  HIPCHK(hipGetLastError());
  { const int rc = scan_in_place(d_P, R + 1); if (rc != SVDSS_OK) return rc; }
  L.ms[1] = since(t0);
  // ---- chain
  t0 = std::chrono::steady_clock::now();
  uint32_t *d_table = nullptr, *d_entry_state = nullptr;
  int64_t *d_entry_block = nullptr, *d_res = nullptr;
  int32_t* d_flag = nullptr;
  HIPCHK(B_.get(&d_table, (size_t)n_tiles * ENTRY_STATES * 4));
  HIPCHK(B_.get(&d_entry_state, (size_t)n_tiles * 4));
  HIPCHK(B_.get(&d_entry_block, (size_t)n_tiles * 8));
  HIPCHK(B_.get(&d_res, 16));
  HIPCHK(B_.get(&d_flag, 8));
  HIPCHK(hipMemset(d_flag, 0, 8));
  hipLaunchKernelGGL(k_tables, dim3(grid_for(n_tiles * ENTRY_STATES)), dim3(256), 0, 0, d_start, d_P, R, T, n_tiles, d_table);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_walker, dim3(1), dim3(64), 0, 0, d_table, d_start, d_P, R, T, n_tiles, piece_words, d_entry_state, d_entry_block, d_res);
  HIPCHK(hipGetLastError());
  int64_t res[2] = {0, 0};
  HIPCHK(hipMemcpy(res, d_res, 16, hipMemcpyDeviceToHost));
  const int64_t NB = res[0];   // data blocks; block NB is the closing header
  if (res[1] || NB <= 0 || NB > R) { g_svdss_hip_err = "rld0 device encoder: the chain of block starts left its tables"; return SVDSS_EHIP; }
  // 72 bytes per block: descriptor 8, data words 64
  if (!fits((size_t)(NB + 2) * 72)) return -SVDSS_FMD_DECLINED_MEMORY;
  int64_t* d_desc = nullptr;
  uint64_t* d_out = nullptr;
  HIPCHK(B_.get(&d_desc, (size_t)(NB + 2) * 8));
  hipLaunchKernelGGL(k_desc, dim3(grid_for(n_tiles)), dim3(256), 0, 0, d_start, d_P, R, T, n_tiles, piece_words, d_entry_state, d_entry_block,
                     NB, decline_syms, d_desc, d_flag);
  HIPCHK(hipGetLastError());
  int32_t flag[2] = {0, 0};
  HIPCHK(hipMemcpy(flag, d_flag, 8, hipMemcpyDeviceToHost));
  if (flag[1]) { g_svdss_hip_err = "rld0 device encoder: the tiles' walks and the walker disagree"; return SVDSS_EHIP; }
  L.ms[2] = since(t0);
  if (flag[0]) return -SVDSS_FMD_DECLINED_BLOCK;
  int64_t closing = 0;
  HIPCHK(hipMemcpy(&closing, d_desc + NB, 8, hipMemcpyDeviceToHost));
  const int64_t k = NB * RLD0_BLOCK_WORDS + rld0_hdr_words((int)((uint64_t)closing >> 62));
  // ---- emit
  t0 = std::chrono::steady_clock::now();
  HIPCHK(B_.get(&d_out, (size_t)(NB + 1) * 64));
  hipLaunchKernelGGL(k_emit, dim3(grid_for(NB + 1)), dim3(256), 0, 0, d_start, d_sym, R, d_desc, NB, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  L.ms[3] = since(t0);
  // ---- download + write
  t0 = std::chrono::steady_clock::now();
  const int64_t slice_words = std::max<int64_t>(RLD0_BLOCK_WORDS, env_i64("SVDSS_FMD_SLICE_WORDS", (int64_t)4 << 20) / RLD0_BLOCK_WORDS * RLD0_BLOCK_WORDS);
  uint64_t* h[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) { HIPCHK(hipHostMalloc((void**)&h[i], (size_t)slice_words * 8)); B_.pinned.push_back(h[i]); }
  hipStream_t st = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  Rld0Frames fr;
  fr.begin((uint64_t)n, k);
  uint64_t mcnt[6];
  for (int c = 0; c < 6; ++c) mcnt[c] = (uint64_t)(acc[c + 1] - acc[c]);
  FILE* f = fopen(path, "wb");
  if (!f) { (void)hipStreamDestroy(st); return SVDSS_EIO; }
  bool ok = rld0_write_header(f, k, fr.n_frames, mcnt);
  hipError_t he = hipSuccess;
  const int64_t n_slices = (k + slice_words - 1) / slice_words;
  auto words_of = [&](int64_t s) { return std::min(slice_words, k - s * slice_words); };
  if (n_slices > 0) he = hipMemcpyAsync(h[0], d_out, (size_t)words_of(0) * 8, hipMemcpyDeviceToHost, st);
  for (int64_t s = 0; s < n_slices && ok && he == hipSuccess; ++s) {
    he = hipStreamSynchronize(st);
    if (he != hipSuccess) break;
    if (s + 1 < n_slices) he = hipMemcpyAsync(h[(s + 1) & 1], d_out + (s + 1) * slice_words, (size_t)words_of(s + 1) * 8, hipMemcpyDeviceToHost, st);
    const uint64_t* z = h[s & 1];
    ok = fwrite(z, 8, (size_t)words_of(s), f) == (size_t)words_of(s);
    fr.feed(z, s * slice_words, words_of(s));
  }
  (void)hipStreamSynchronize(st);
  (void)hipStreamDestroy(st);
  fr.finish();
  ok = ok && he == hipSuccess && fwrite(fr.frame.data(), 8, fr.frame.size(), f) == fr.frame.size();
  ok = (fclose(f) == 0) && ok;
  if (he != hipSuccess) { g_svdss_hip_err = std::string("rld0 device encoder, download: ") + hipGetErrorString(he); return SVDSS_EHIP; }
  if (!ok) return SVDSS_EIO;
  L.ms[4] = since(t0);
  L.ms[5] = since(t_all);
  L.route = SVDSS_FMD_DEVICE;
  L.runs = R;
  L.blocks = NB;
  L.pieces = (k + piece_words - 1) / piece_words;
  g_last = L;
  if (getenv("SVDSS_DEBUG")) fprintf(stderr, "fmd: %.1f ms of the stages' times are hipMalloc / hipFree\n", B_.alloc_ms);
  return SVDSS_OK;
}

// the device encoder on blocks that are on the host: uploaded to `device` first
int rld0_dev_encode_host_blocks(const svdss_index* ix, int device, const char* path) {
  if (ix->n <= 0) return -SVDSS_FMD_DECLINED_EMPTY;
  if (getenv("SVDSS_INDEX_CPU")) return -SVDSS_FMD_DECLINED_NO_GPU;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device >= count) { (void)hipGetLastError(); return -SVDSS_FMD_DECLINED_NO_GPU; }
  HIPCHK(hipSetDevice(device));
  const size_t bb = ix->blocks.size() * sizeof(svdss_u4);
  if (!fits(bb)) return -SVDSS_FMD_DECLINED_MEMORY;
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, bb));
  int rc = hipMemcpy(d, ix->blocks.data(), bb, hipMemcpyHostToDevice) == hipSuccess ? SVDSS_OK : SVDSS_EHIP;
  if (rc == SVDSS_OK) rc = rld0_dev_encode(d, ix->n, ix->acc, path);
  (void)hipFree(d);
  return rc;
}

extern "C" int svdss_fmd_encode(const uint8_t* bwt, int64_t n, const char* path, int device) {
  if (!path || n < 0 || (!bwt && n > 0) || device < -1) return SVDSS_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = -SVDSS_FMD_HOST;
  if (device >= 0) {
    for (int64_t i = 0; i < n; ++i)
      if (bwt[i] > 5) return SVDSS_EINVAL;
    svdss_index tmp;
    if (n > 0) { rc = svdss_blocks_from_bwt(bwt, n, 4, &tmp); if (rc != SVDSS_OK) return rc; }
    rc = rld0_dev_encode_host_blocks(&tmp, device, path);
    if (rc >= 0) return rc;   // written there, or an error
  }
  const int32_t route = -rc;
  rc = rld0_write(path, bwt, n);
  rld0_encode_note(route, since(t0));
  return rc;
}

extern "C" int svdss_fmd_encode_last(int32_t* route, int64_t* runs, int64_t* blocks, int64_t* pieces, double ms[6]) {
  if (g_last.route < 0) return SVDSS_ENODEV;
  if (route) *route = g_last.route;
  if (runs) *runs = g_last.runs;
  if (blocks) *blocks = g_last.blocks;
  if (pieces) *pieces = g_last.pieces;
  if (ms) memcpy(ms, g_last.ms, sizeof g_last.ms);
  return SVDSS_OK;
}
