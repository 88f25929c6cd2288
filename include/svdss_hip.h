/*
 * svdss_hip.h -- C ABI of the MI355X-native SVDSS hot path (libsvdss_hip.so).
 *
 * Drop-in boundary B2 of SURVEY.md section 8(b): the reference (Parsoa/SVDSS
 * v2.1.1) has no plugin layer; the seam is where its stage drivers call into
 * per-item kernels and third-party C functions.  Each entry point below cites
 * the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions: plain-old-data in and out, caller-owned buffers, int status
 * return (0 = ok; the host turns non-zero into a stderr message + exit(1)
 * like ping_pong.cpp:62-63), no exceptions across the ABI, no torch types.
 * Symbols use ropebwt3's nt6 alphabet: $=0 A=1 C=2 G=3 T=4 N/other=5.
 */
#ifndef SVDSS_HIP_H
#define SVDSS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVDSS_OK 0
#define SVDSS_EINVAL 1    /* bad argument */
#define SVDSS_ENOMEM 2    /* host or device allocation failed */
#define SVDSS_EIO 3       /* file could not be read/written or has a bad format */
#define SVDSS_EHIP 4      /* a HIP runtime call failed (no GPU, launch error, ...) */
#define SVDSS_ENODEV 5    /* index is not resident on a device */
#define SVDSS_ERANGE 6    /* input exceeds a layout limit (per-symbol count >= 2^32, read >= 2^31) */

const char* svdss_strerror(int code);
/* Last HIP error string seen by this library on the calling thread ("" if none). */
const char* svdss_last_hip_error(void);

/* ---- a1: base -> nt6 ----------------------------------------------------
 * Replaces seq_nt6_table (ping_pong.hpp:46-52) as applied at
 * ping_pong.cpp:90-94 (BAM path) and rb3_char2nt6 at ping_pong.cpp:158. */
int svdss_nt6_encode(const char* seq, int64_t n, uint8_t* out);

/* ---- a5: FM-index -------------------------------------------------------
 * svdss_index_build replaces `ropebwt3 build` re-exported as `SVDSS index`
 * (main.cpp:15-17,34-37); svdss_index_load replaces rb3_fmi_restore
 * (ping_pong.cpp:245).  contigs = concatenated nt6 symbols of all records,
 * lens[i] symbols each.  The index covers every record and its reverse
 * complement, each '$'-terminated.  The index is built in HBM; a machine without a GPU gets SVDSS_EHIP ("no GPU
 * found"), not a quiet run of the host builder -- that one serves the texts the GPU builder refuses and
 * SVDSS_INDEX_CPU=1. */
typedef struct svdss_index svdss_index_t;

int svdss_index_build(const uint8_t* contigs, const int64_t* lens, int32_t n_contigs,
                      int32_t threads, svdss_index_t** out);
/* The same index built directly in the HBM of `device` and left resident there, k-mer table included
 * (csrc/index_gpu.hip: text, suffix sorting, BWT and rank blocks on the GPU; GRCh38 lengths in tens of seconds
 * instead of minutes of host cores).  Text and suffix array stay on the device -- svdss_index_save fetches them
 * when asked.  Falls back to svdss_index_build + svdss_index_to_device when the device lacks the memory.
 * This is what every rank of a multi-GPU run calls for its own replica (index replicated). */
int svdss_index_build_device(const uint8_t* contigs, const int64_t* lens, int32_t n_contigs,
                             int32_t threads, int32_t device, svdss_index_t** out);
int svdss_index_save(const svdss_index_t* ix, const char* path);
/* The records file (magic "SVDSSRC1": BWT length, acc[], record lengths, the nt6 records): what `SVDSS index` leaves
 * beside the .fmd as `<fmd>.svdss`.  svdss_index_load takes it and returns an index that holds the records only; the
 * layout is built when the index is made resident (svdss_index_to_device / svdss_index_replicate: in the HBM of that
 * device, seconds for GRCh38 lengths -- faster than any disk delivers the 58 GB of text + suffix array
 * svdss_index_save writes) or when a host-side accessor needs it.  Stands where the .fmd stands between main_build and
 * rb3_fmi_restore (main.cpp:34-37, ping_pong.cpp:245). */
int svdss_index_save_records(const svdss_index_t* ix, const char* path);
/* The index as ropebwt3 dumps it: the rld0 run-length BWT (`.fmd`, magic "RLD\3"), the file `ropebwt3 build -d` /
 * upstream `SVDSS index` writes and rb3_fmi_restore reads (main.cpp:34-37, ping_pong.cpp:245; run_svdss:136-147 reuses
 * an existing $FA.fmd).  Format restated from the published rld0 sources in csrc/rld0.cpp [UPSTREAM-UNVERIFIED]. */
int svdss_index_save_fmd(const svdss_index_t* ix, const char* path);
/* The BWT an rld0 `.fmd` holds, as nt6 bytes: *n_out symbols (bwt_out may be NULL to ask for the size only;
 * SVDSS_ERANGE if cap is too small). */
int svdss_fmd_read_bwt(const char* path, uint8_t* bwt_out, int64_t cap, int64_t* n_out);
/* The rld0 `.fmd` of a BWT (nt6 bytes, '$' = 0) -> path.  device >= 0: rank blocks of the BWT built on the host, uploaded,
 * and the file encoded on that GPU (csrc/rld0_dev.hip: run starts from the bit planes, the chain of block starts by tile
 * tables, a lane per 64-byte block) -- the bytes the host encoder writes; device == -1: the host encoder (csrc/rld0.cpp).
 * The device declines whole calls, never part of a file -- the host encoder then writes it: an empty BWT, a block of
 * SVDSS_FMD_DECLINE_SYMS (default and at most 2^30) symbols or more, a plan that does not fit in free HBM, no GPU or
 * SVDSS_INDEX_CPU set. */
int svdss_fmd_encode(const uint8_t* bwt, int64_t n, const char* path, int device);
/* How the calling thread's last .fmd encode (svdss_fmd_encode, svdss_index_save_fmd, svdss_index_save_fmd_on) ran:
 * *route one of SVDSS_FMD_*; on the device also its runs, data blocks and pieces of 2^23 words, and ms[0..4] = the
 * milliseconds of the stages planes, plan, chain, emit, download + write; ms[5] = the whole call.  SVDSS_ENODEV before the
 * first encode. */
#define SVDSS_FMD_HOST 0              /* the host encoder, as asked (device -1, SVDSS_FMD_ENCODE_DEVICE=0) */
#define SVDSS_FMD_DEVICE 1            /* the device encoder */
#define SVDSS_FMD_DECLINED_EMPTY 2    /* declined: n == 0 */
#define SVDSS_FMD_DECLINED_BLOCK 3    /* declined: a block of SVDSS_FMD_DECLINE_SYMS symbols or more */
#define SVDSS_FMD_DECLINED_MEMORY 4   /* declined: the plan does not fit in free HBM */
#define SVDSS_FMD_DECLINED_NO_GPU 5   /* declined: no GPU, or SVDSS_INDEX_CPU set */
int svdss_fmd_encode_last(int32_t* route, int64_t* runs, int64_t* blocks, int64_t* pieces, double ms[6]);
/* svdss_index_save_fmd with the encoder named: device >= 0 the device encoder on that GPU (from the resident rank blocks
 * where the handle is resident there, else its host blocks are uploaded), -1 the host encoder, -2 what
 * svdss_index_save_fmd does: SVDSS_FMD_ENCODE_DEVICE=1 or unset the device (where the handle is resident, else GPU 0;
 * the default since profiles/fmd_encode.txt), 0 the host. */
int svdss_index_save_fmd_on(const svdss_index_t* ix, const char* path, int32_t device);
/* The strings of the collection a BWT stands for (nt6, '$' = 0 in `bwt`): string r is the one spelled from row r;
 * they are written back to back into out (n - m bytes), their lengths into lens.  device >= 0: rank blocks built
 * and walked there (csrc/bwt_invert.hip: marked LF walks, a walker per lane; the same walk on the host where HBM has
 * no room); device < 0: the same walk on the host.  stride: the distance of the marked rows at which the walks are cut;
 * 0 = SVDSS_INVERT_STRIDE or the default; the result never depends on it.  stride < 0 (host only): one serial walk
 * per string without a step limit -- what a caller takes after SVDSS_ERANGE for the limit.
 * SVDSS_EINVAL: a null pointer, n <= 0, a symbol above 5.  SVDSS_ERANGE with *n_strings = the number of strings: a
 * capacity is too small; SVDSS_ERANGE otherwise: a walker passed SVDSS_INVERT_MAX_STEPS steps, or a symbol occurs 2^32
 * times or more.  SVDSS_EIO: not the BWT of a string collection (a walker on no chain or on two, lengths that do not sum
 * to n - m). */
int svdss_bwt_strings(const uint8_t* bwt, int64_t n, int32_t device, int64_t stride,
                      uint8_t* out, int64_t out_cap, int64_t* lens, int32_t lens_cap, int32_t* n_strings);
/* How the calling thread's last svdss_bwt_strings ran: *route 0 = the marked walks on the host, 1 = on the device,
 * 2 = the serial walk per string; its stride and walkers; ms[3] = milliseconds of the rank blocks' build, pass 1, pass 2
 * (route 2: everything in ms[1]).  SVDSS_ENODEV before the first call. */
int svdss_bwt_strings_last(int32_t* route, int64_t* stride, int64_t* walkers, double* ms);
/* Restores an index: this library's own files (svdss_index_save, svdss_index_save_records), or an rld0 `.fmd` -- then
 * `<path>.svdss` (the file `SVDSS index` leaves beside the .fmd) is read if it is there, not older, and carries the
 * symbol counts of the .fmd's header; otherwise the BWT is
 * decoded, the records are recovered from it (they must come with their reverse complements, as ropebwt3 build -d
 * inserts them) and the index is rebuilt on the GPU (no GPU: SVDSS_EHIP, unless SVDSS_INDEX_CPU=1 asks for the host
 * builder). */
int svdss_index_load(const char* path, svdss_index_t** out);
/* The records an index file stands for, without building the index (`SVDSS index -i OLD`): a handle that holds
 * them, from the sidecar `path`.svdss (or `path` itself, this library's layout) where svdss_index_load would read
 * that, else out of the .fmd's BWT: svdss_bwt_strings on `device` (< 0: on the host), one string of every
 * reverse-complement pair.  *source: 0 records sidecar, 1 full layout, 2 device walk, 3 host walk, 4 the serial walk per
 * string (SVDSS_FMD_IMPORT_DEVICE=0, or past the step limit).  Errors as svdss_index_load reports them. */
int svdss_index_records_open(const char* path, int32_t device, svdss_index_t** out, int32_t* source);
/* The records a handle holds (nt6, back to back) and their lengths: pointers into the handle, valid until it is freed
 * or made resident.  SVDSS_ENODEV: it holds none. */
int svdss_index_records(const svdss_index_t* ix, const uint8_t** records, const int64_t** lens, int32_t* n_records);
void svdss_index_free(svdss_index_t* ix);
/* number of BWT symbols, = sum_i 2*(lens[i]+1) */
int64_t svdss_index_size(const svdss_index_t* ix);
/* acc[c] = number of symbols < c (rb3_fmi_t::acc, used by rb3_fmd_set_intv) */
int svdss_index_acc(const svdss_index_t* ix, int64_t acc[7]);
/* decode the BWT as nt6 bytes (svdss_index_size() of them) */
int svdss_index_bwt(const svdss_index_t* ix, uint8_t* bwt_out);
/* bytes the index occupies in HBM once resident */
int64_t svdss_index_device_bytes(const svdss_index_t* ix);
/* order K of the k-mer table built by svdss_index_to_device (0 before / without it) */
int32_t svdss_index_kmer(const svdss_index_t* ix);
/* The index as a rank structure alone.  `SVDSS index` leaves the rank blocks and '$' rows behind the records of its
 * sidecar; svdss_index_attach_blocks (before svdss_index_to_device, on a handle svdss_index_load gave for the same path)
 * makes them the handle's host side and drops the records: svdss_index_to_device then uploads ~n/2 bytes instead of
 * rebuilding text, suffix array and k-mer table (rb3_fmi_restore, ping_pong.cpp:245, restores exactly this much: the
 * reference searches with rank steps alone).  The search is then one rank step per rb3_fmd_extend -- about a million reads
 * per second at GRCh38 lengths instead of 8 - 24 M, results identical -- which pays when few reads are searched.
 * SVDSS_EINVAL: the file has no such section (restore as before). */
int svdss_index_attach_blocks(svdss_index_t* ix, const char* path);
int svdss_index_load_blocks(const char* path, svdss_index_t** out);       /* the same as a handle of its own: the records are never read */
int svdss_index_append_blocks(const svdss_index_t* ix, const char* path);   /* behind the records svdss_index_save_records wrote at `path` */
/* An upper limit for the order of tables built FROM NOW ON (process-wide; 0 = none; an explicit SVDSS_KMER wins).  The
 * table's build time quarters per step down, the search kernel slows down by about a factor of two per step: a process that
 * restores the index for one input may learn, while the suffix array is still being sorted, that it has few reads to search
 * (`SVDSS search` on a smoothed BAM: the putative filter of ping_pong.cpp:202-203 skips most of them) -- the limit is read
 * when the table's build begins.  Results never depend on K. */
void svdss_index_kmer_limit(int32_t k);
/* share of the k-mer occurrences (sampled while the table is built) that belong to k-mers with 8 or more of them: a
 * reference rich in young repeat families has >= 0.35, and the search then finishes backward phases on deep intervals by
 * binary search of the suffix array (the BS instantiation of the kernel; SVDSS_BS=0|1 overrides, SVDSS_BS_DEEP moves the
 * threshold).  Results never depend on it. */
double svdss_index_deep_frac(const svdss_index_t* ix);
/* copy the index into the HBM of `device` (replicated per GPU): BWT blocks,
 * text, suffix array, and the 4^K k-mer table (K = floor(log4 n)+1, env SVDSS_KMER overrides) */
int svdss_index_to_device(svdss_index_t* ix, int32_t device);

/* A resident index checked against its own text by direct comparison, independently of how it was built
 * (csrc/index_verify.hip): every `stride`-th suffix-array row i has SA[i] in range, text[SA[i]..) < text[SA[i+1]..)
 * as strings, BWT[i] == text[SA[i]-1]; every rank block's counters continue the previous block's; the '$' rows are
 * the listed ones; the text's symbol histogram is acc[].  stride 1 = the whole index (GRCh38 lengths: ~1 s).
 * out[0] rows checked, [1] order violations, [2] BWT mismatches, [3] entries out of range, [4] block / histogram
 * violations, [5] '$'-list violations, [6] first bad row or -1, [7] longest common prefix met.  The index this
 * stands for is the one rb3_fmi_restore returns (ping_pong.cpp:245). */
int svdss_index_verify_device(const svdss_index_t* ix, int64_t stride, int64_t out[8]);

/* GPUs this process sees (0: none). */
int svdss_device_count(void);
/* Free and total memory of `device` as the runtime reports them now (hipMemGetInfo): what `SVDSS run --samples` prints at
 * the start of every sample with --verbose, and what it decides on whether the index stays resident through the call stage. */
int svdss_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);
/* A stream of the kind the library makes for its own searches, for callers that pass their stream to
 * svdss_sfs_search_batch_device (bench.py): non-blocking, and restricted to the compute units SVDSS_SEARCH_CUS names
 * ("first,count": bits of hipExtStreamCreateWithCUMask's mask; csrc/hip_check.h) when that is set.  The call-side
 * batch objects do the same with SVDSS_CALL_CUS: kernels that each fill the chip run side by side on disjoint CUs
 * instead of taking turns (no counterpart in the reference: its threads share cores the same way through OpenMP). */
int svdss_search_stream_create(int32_t device, void** stream);
int svdss_stream_destroy(void* stream);
/* One more replica of the index, in the HBM of `device` (the index is replicated per GPU, reads and
 * sub-clusters shard): a new handle with its own device buffers; *src is not modified (its text and suffix array are
 * fetched to the host first if it was built on a device). */
int svdss_index_replicate(const svdss_index_t* src, int32_t device, svdss_index_t** out);

/* Size of the interval of a pattern (occurrences in contigs + revcomps) via
 * the host copy of the index; rb3_fmd_set_intv + repeated rb3_fmd_extend(...,1)
 * as in ping_pong.cpp:12-22.  For tests/diagnostics; not a hot path. */
int64_t svdss_index_count(const svdss_index_t* ix, const uint8_t* pattern_nt6, int64_t len);

/* ---- a2+a3+a4 (+a8): batched ping-pong SFS search -----------------------
 * Replaces PingPong::ping_pong_search (ping_pong.hpp:84-85, ping_pong.cpp:4-49)
 * called per read from PingPong::process_batch (ping_pong.cpp:176-209), i.e.
 * the rb3_fmd_set_intv / rb3_fmd_extend loops, for a whole batch at once.
 *
 * reads    : concatenated nt6 symbols; read i = reads[offsets[i] .. offsets[i+1])
 *            (no terminator byte needed; the P[l]=0 of ping_pong.cpp:94 is implied)
 * flags    : SVDSS_SFS_ASSEMBLE applies Assembler::assemble (assembler.cpp:34-56)
 *            per read as ping_pong.cpp:219-222 does unless --noassemble.
 * Results per read i: counts[i] records (qs,len); without ASSEMBLE in the
 * order ping_pong.cpp:41 pushes them (descending qs), with ASSEMBLE ascending
 * qs (assembler.cpp:36).  n_ext[i] = number of rb3_fmd_extend calls the
 * reference would have made for that read (ping_pong.cpp:20,35).
 * overlap is fixed at -1 (config.hpp:87; the option is never declared,
 * config.cpp:30-55,74). */
#define SVDSS_SFS_ASSEMBLE 1

typedef struct svdss_sfs_batch svdss_sfs_batch_t;

/* Host-buffer entry point: uploads, searches on the index's device, leaves
 * results in *out (created if *out == NULL, otherwise its buffers are reused). */
int svdss_sfs_search_batch(const svdss_index_t* ix, const uint8_t* reads, const int64_t* offsets,
                           int64_t n_reads, int32_t flags, svdss_sfs_batch_t** out);
/* BAM-record entry point: the reads as they sit in BAM records -- 4-bit packed bases ("=ACMGRSVTWYHKDBN", two per
 * byte, high nibble first), read i at seq4[byte_off[i]] with l_seq[i] bases -- are uploaded packed (half the bytes of
 * the nt6 form) and expanded to nt6 on the GPU, which stands for the per-base loop of ping_pong.cpp:90-94
 * (seq_nt16_str, then seq_nt6_table: A/C/G/T -> 1..4, every other code -> 5).  Everything else as
 * svdss_sfs_search_batch.  Copies go through the batch object's own stream: calls on different batch objects overlap. */
int svdss_sfs_search_batch_bam(const svdss_index_t* ix, const uint8_t* seq4, const int64_t* byte_off,
                               const int32_t* l_seq, int64_t n_reads, int32_t flags, svdss_sfs_batch_t** out);
/* Page-locked host memory for the buffers handed to the host-buffer entry points (copies from it run at PCIe speed
 * and asynchronously; pageable memory works too, slower). */
int svdss_host_alloc(int64_t bytes, void** out);
void svdss_host_free(void* p);
/* ---- BGZF blocks inflated on the GPU (csrc/inflate.hip).  Stands where htslib's bgzf_read / inflate stand under
 * sam_read1 (/root/reference/ping_pong.cpp:58,247-249): every BGZF block is an independent deflate stream of at most
 * 64 KB, one wavefront inflates one block.  `comp` holds the compressed bytes (host memory, page-locked for speed);
 * block i is the raw deflate stream comp[coff, coff + clen) and inflates to exactly isize bytes at d_out + uoff (d_out: a
 * device buffer of out_bytes bytes, e.g. from svdss_device_alloc).  If host_out is not NULL the inflated bytes are also
 * copied there.  Returns when everything is done (work runs on the object's own stream: calls on different objects
 * overlap).  A block that does not inflate to isize bytes gives SVDSS_EIO and its index in *bad_block; the CRC32 of the
 * BGZF footer is NOT checked on this path. */
typedef struct svdss_inflate svdss_inflate_t;
typedef struct svdss_bgzf_block {
  int64_t coff;    /* first byte of the deflate stream in comp */
  int32_t clen;    /* its length */
  int32_t isize;   /* inflated size (BGZF footer), 0..65536 */
  int64_t uoff;    /* where the block inflates to, relative to d_out */
} svdss_bgzf_block_t;
int svdss_bgzf_inflate(svdss_inflate_t** obj, int device, const uint8_t* comp, int64_t comp_bytes,
                       const svdss_bgzf_block_t* blocks, int64_t n_blocks, void* d_out, uint8_t* host_out,
                       int64_t out_bytes, int64_t* bad_block);
double svdss_inflate_kernel_ms(const svdss_inflate_t* obj);   /* the inflate kernel of the last call, HIP events */
void svdss_inflate_free(svdss_inflate_t* obj);
/* ---- BGZF blocks DEFLATED on the GPU (csrc/deflate.hip).  Stands where htslib's bgzf_write / deflate stand under
 * sam_write1 in `SVDSS smooth` (/root/reference/smoother.cpp:441-494).  `in` (host memory) is cut into blocks of
 * block_bytes (<= 0xff00; the last one may be short); block i becomes a BGZF member at out + i * out_stride (host
 * memory; out_stride >= block_bytes + 64, a multiple of 4): 18-byte header with BSIZE, a deflate stream of dynamic-
 * Huffman coded literals and runs (4, 8, ... 256 equal bytes as one match at distance 1; no other matches: a
 * level-1-class encoder for packed bases and qualities; incompressible quarters are stored), and 8 bytes LEFT FOR THE CALLER to fill with CRC32 and ISIZE; out_len[i] = the member's length with
 * those 8 bytes.  out_stride 0: the members are written back to back instead (out needs in_bytes + 64 per block).
 * Any inflater reads the result; it is not the byte stream zlib would write.  Returns when done (the
 * object's own stream: calls on different objects overlap).
 * svdss_bgzf_deflate_mode: the same with the encoder's mode.  SVDSS_DEFLATE_RUNS (0) is svdss_bgzf_deflate, byte for
 * byte.  SVDSS_DEFLATE_LZ (1) adds general matches (length 4..258, distance 1..32768, never in front of the member's own
 * first byte; a distance code of its own per quarter): what a coordinate-sorted BAM repeats from one overlapping read to
 * the next, a record (~22 KB) back.  A match finder kernel runs in front of the coder; the container is the same. */
typedef struct svdss_deflate svdss_deflate_t;
#define SVDSS_DEFLATE_RUNS 0
#define SVDSS_DEFLATE_LZ 1
int svdss_bgzf_deflate(svdss_deflate_t** obj, int32_t device, const uint8_t* in, int64_t in_bytes, int32_t block_bytes,
                       uint8_t* out, int64_t out_stride, int32_t* out_len);
int svdss_bgzf_deflate_mode(svdss_deflate_t** obj, int32_t device, const uint8_t* in, int64_t in_bytes, int32_t block_bytes,
                            uint8_t* out, int64_t out_stride, int32_t* out_len, int32_t mode);
double svdss_deflate_kernel_ms(const svdss_deflate_t* obj);
void svdss_deflate_free(svdss_deflate_t* obj);
/* plain device memory for the callers of the entry points that take device pointers */
int svdss_device_alloc(int device, int64_t bytes, void** out);
void svdss_device_free(int device, void* p);
int svdss_device_memset(int device, void* d_dst, int value, int64_t bytes);
int svdss_device_download(int device, void* dst, const void* d_src, int64_t bytes);
/* Device-buffer entry point: d_reads/d_offsets already resident in HBM on the
 * index's device; work is enqueued on `stream` (a hipStream_t, NULL = default
 * stream) and is complete when this returns. */
int svdss_sfs_search_batch_device(const svdss_index_t* ix, const uint8_t* d_reads,
                                  const int64_t* d_offsets, int64_t n_reads, int64_t total_syms,
                                  int32_t flags, void* stream, svdss_sfs_batch_t** out);
int64_t svdss_sfs_batch_nreads(const svdss_sfs_batch_t* b);
int64_t svdss_sfs_batch_total(const svdss_sfs_batch_t* b);       /* sum of counts */
int64_t svdss_sfs_batch_total_ext(const svdss_sfs_batch_t* b);   /* sum of n_ext */
/* Small batches are searched with several lanes per read (segments stitched exactly, see
 * DESIGN.md); these report the segment count the last call used (1 = one lane per read) and
 * how many reads had to be redone unsegmented because their chains could not be stitched. */
int32_t svdss_sfs_batch_segments(const svdss_sfs_batch_t* b);
int64_t svdss_sfs_batch_fallbacks(const svdss_sfs_batch_t* b);
int32_t svdss_sfs_batch_used_bs(const svdss_sfs_batch_t* b);   /* 1: the last call launched the BS instantiation */
/* duration of the search kernel(s) of the last call, from HIP events on its stream */
double svdss_sfs_batch_kernel_ms(const svdss_sfs_batch_t* b);
/* HIP-event time of the search kernel alone (first pass; without ordering, stitching, assembling, gather) */
double svdss_sfs_batch_search_kernel_ms(const svdss_sfs_batch_t* b);
/* copy results to host; any pointer may be NULL to skip it.
 * counts,n_ext: n_reads entries; qs,len: svdss_sfs_batch_total() entries. */
int svdss_sfs_batch_fetch(const svdss_sfs_batch_t* b, int64_t* counts, int32_t* qs, int32_t* len,
                          int64_t* n_ext);
/* device addresses of the result arrays (valid until the next search on this batch
 * object or svdss_sfs_batch_free): counts int64[n_reads], qs/len int32[total],
 * n_ext int64[n_reads].  Lets a caller hand results to RCCL without a host hop. */
int svdss_sfs_batch_device_ptrs(const svdss_sfs_batch_t* b, void** counts, void** qs, void** len,
                                void** n_ext);
void svdss_sfs_batch_free(svdss_sfs_batch_t* b);

/* ---- a6 + a7 on the device: BAM records in, SFS out (csrc/bam_device.hip) ------------------------------------
 * Replaces PingPong::load_batch_bam (ping_pong.cpp:53-128: sam_read1 = BGZF inflate + the block_size chain of the
 * records, the flag / l_qseq / tid filters :66-79, 4-bit -> nt6 :90-94) and the head of PingPong::process_batch (:196-203:
 * bam_aux_get("XF"/"HP"), the putative filter) for a run of consecutive BGZF blocks at once, followed by the search of
 * svdss_sfs_search_batch_device.  Only compressed bytes go up; names, tags and SFS come down.
 *
 * A svdss_bam_stream_t is one BAM file being read: it holds the bytes of the record that straddles two consecutive
 * batches and gives the batches their turn in file order (everything else of a batch -- inflate, the record chain of
 * its segments, unpack, search -- overlaps with the other batches, each on its own svdss_bam_batch_t / stream / thread).
 * n_ref = reference sequences in the BAM header (tid / mtid outside -1 .. n_ref - 1 never start a record).
 *
 * svdss_bam_batch_run, batch number seq = 0, 1, 2, ... of the file (every number exactly once, from any thread; is_last on
 * the final one): n_chunks pieces of the file in page-locked or ordinary host memory; piece c holds n_blocks[c] BGZF
 * blocks, block i = the raw deflate stream comp[c][coff, coff + clen) that inflates to isize bytes with CRC32 crc[c][i]
 * (uoff is ignored: the blocks of a batch inflate back to back in the order given).  skip = inflated bytes in front of the
 * first record (the BAM header; batch 0 only).  flags: SVDSS_SFS_ASSEMBLE, SVDSS_BAM_PUTATIVE (reads whose XF tag is not 0
 * keep their slot but are not searched, ping_pong.cpp:202-203).
 * Errors: SVDSS_EIO with svdss_bam_batch_error() = "BGZF inflate failed" | "BGZF block CRC mismatch" | "truncated record" |
 * "corrupt record" | "core.tid < 0. Why are we here? Please check" (the reference's fatal message, :76-79); once a batch
 * failed every later batch of the stream returns its error. */
typedef struct svdss_bam_stream svdss_bam_stream_t;
typedef struct svdss_bam_batch svdss_bam_batch_t;
#define SVDSS_BAM_PUTATIVE 0x100
/* Added to `skip` of a batch other than 0 (every entry point that runs a batch): the batch begins a RANGE of the file of its
 * own, behind a gap -- at a known record start, skip bytes into its first member.  The bytes the batch in front carried
 * (the record cut at its range's end) are dropped and the chain starts there.  The stream must be open at its end
 * (svdss_bam_stream_region).  `--region` with an index reads the ranges the index names as ONE stream this way. */
#define SVDSS_BAM_SKIP_RESTART ((int64_t)1 << 40)
int svdss_bam_stream_create(int32_t n_ref, svdss_bam_stream_t** out);
void svdss_bam_stream_free(svdss_bam_stream_t* s);
const char* svdss_bam_stream_error(const svdss_bam_stream_t* s);
/* A stream over a REGION of the file (`SVDSS search --gpus N` gives every GPU its own range of BGZF blocks -- north_star:
 * "BAM regions partition across the GPUs"; the per-shard loop of ping_pong.cpp:53-128).  Call before batch 0.
 * open_start: the region begins inside a record nobody has located yet: batch 0 starts the chain at the first record its
 *   segments guess (plausible fields, a plausible record behind it) and keeps the bytes in front of it (svdss_bam_stream_head).
 *   The guess is proved by the caller: the previous region's tail + this head must be a chain of whole records -- run
 *   them as a one-batch stream of their own; if they are not, run the region again with open_start = 0 and carry = the
 *   previous region's tail (the incomplete record in front of batch 0).
 * open_end: the last batch may end inside a record; svdss_bam_stream_tail are its bytes (no "truncated record"). */
int svdss_bam_stream_region(svdss_bam_stream_t* s, int32_t open_start, int32_t open_end, const uint8_t* carry, int64_t n_carry);
int64_t svdss_bam_stream_head(const svdss_bam_stream_t* s, const uint8_t** bytes);   /* after batch 0 */
int64_t svdss_bam_stream_tail(const svdss_bam_stream_t* s, const uint8_t** bytes);   /* after the last batch */
/* The record gate (`--region` / `--regions-file`).  Call before batch 0.  n intervals [beg, end) (0-based, half open) of
 * references tid, sorted by (tid, beg) and merged (on one reference each begins at or behind the end of the one before);
 * n = 0: no record is in.  From then on every entry point that runs a batch of the stream -- svdss_bam_batch_front / _run,
 * svdss_bam_select_run / _select_store_run, svdss_bam_smooth_measure / _run -- sees the batch of a file that holds only the
 * records with tid >= 0 whose [pos, bam_endpos) overlaps an interval of their reference (bam_endpos = pos + the reference
 * length of the CIGAR, pos + 1 where that is 0): the others are no slot, are neither selected nor stored, are dropped by
 * the smoothing.  n_records of a batch's result still counts them; svdss_bam_stream_gated: how many so far. */
int svdss_bam_stream_set_regions(svdss_bam_stream_t* s, int64_t n, const int32_t* tid, const int32_t* beg, const int32_t* end);
int64_t svdss_bam_stream_gated(const svdss_bam_stream_t* s);
int svdss_bam_gated_total(int64_t* out);   /* ... of every stream of the process */
/* segments whose guessed first record the chain did not arrive at (walked again, exactly), of *n_segments in all */
int64_t svdss_bam_stream_rewalked(const svdss_bam_stream_t* s, int64_t* n_segments);
int svdss_bam_batch_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_index_t* ix,
                        int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                        const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                        int32_t flags, svdss_bam_batch_t** out);
/* The two halves of svdss_bam_batch_run, and a PARK for the reads of batches whose front half runs while no index is
 * resident yet: PingPong::run loads the index (ping_pong.cpp:245, seconds for a human genome) and only then starts reading
 * the BAM (:329-363); here the BAM front end (inflate, CRC, record chain, filters, 4-bit -> nt6) runs beside the index
 * restore, the unpacked reads wait in HBM, and are searched in large launches -- one lane per read -- when the index is there.
 *   svdss_bam_batch_front   everything of svdss_bam_batch_run up to the search.  park = NULL, or no room in it, or closed:
 *                           the reads stay in the batch object and svdss_bam_batch_search(b, ix) finishes the batch.
 *                           Else they go into the park (svdss_bam_batch_parked: group >= 0, index of the batch's first
 *                           searched read in the group) and the batch object is free for the next batch; names / tags /
 *                           slots of the batch are on the host either way (svdss_bam_batch_result: counts / qs / len empty).
 *                           group = -2: the batch has no read to search.
 *   svdss_bam_park_create   read_bytes of nt6 symbols + max_reads offsets in the HBM of `device` -- allocate it BEFORE the
 *                           index restore starts so that nothing is handed back to the driver mid-stream.
 *   svdss_bam_park_close    no more reservations (the index is resident); the open group is closed.
 *   svdss_bam_park_search   group g (closed, all its batches unpacked: waits for that) as ONE svdss_sfs_search_batch_device
 *                           launch; results with svdss_sfs_batch_fetch, reads in the order of their reservations.
 * A group closes at SVDSS_PARK_GROUP_READS reads (262,144) or SVDSS_PARK_GROUP_MB of symbols (4,096). */
typedef struct svdss_bam_park svdss_bam_park_t;
int svdss_bam_park_create(int32_t device, int64_t read_bytes, int64_t max_reads, svdss_bam_park_t** out);
void svdss_bam_park_free(svdss_bam_park_t* p);
int svdss_bam_park_close(svdss_bam_park_t* p);
int64_t svdss_bam_park_groups(svdss_bam_park_t* p);
int svdss_bam_park_group(svdss_bam_park_t* p, int64_t g, int64_t* n_batches, int64_t* n_reads, int64_t* n_syms);
int32_t svdss_bam_park_group_ready(svdss_bam_park_t* p, int64_t g);   /* 1: closed and unpacked -- may be searched while later groups still fill */
int svdss_bam_park_search(svdss_bam_park_t* p, int64_t g, const svdss_index_t* ix, int32_t flags, svdss_sfs_batch_t** sfs);
int svdss_bam_batch_front(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int32_t device, svdss_bam_park_t* park,
                          int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                          const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                          int32_t flags, svdss_bam_batch_t** out);
int svdss_bam_batch_parked(const svdss_bam_batch_t* b, int64_t* group, int64_t* first, int64_t* n_reads);
int svdss_bam_batch_search(svdss_bam_batch_t* b, const svdss_index_t* ix);
/* What the last run of a batch object left on the host (valid until its next run / svdss_bam_batch_free).  A "slot" is a
 * record that passed the filters of ping_pong.cpp:66-75, in file order -- what load_batch_bam deals to the threads. */
typedef struct svdss_bam_result {
  int64_t n_records;        /* records of the batch (passed or not) */
  int64_t n_slots;          /* passed the flag and length filters */
  int64_t n_searched;       /* of them searched (all, unless SVDSS_BAM_PUTATIVE) */
  int64_t n_short;          /* dropped for l_qseq < 100 (the reference warns once per read, :70-75) */
  int64_t total_sfs;
  const int32_t* name_off;  /* n_slots + 1: slot i is called names[name_off[i] .. name_off[i + 1]) */
  const char* names;
  const int32_t* hp;        /* n_slots: HP tag, 0 if absent */
  const int32_t* sidx;      /* n_slots: index among the searched reads, -1 = not searched */
  const int64_t* counts;    /* n_searched: SFS per searched read */
  const int32_t* qs;        /* total_sfs, read after read */
  const int32_t* len;
  double inflate_kernel_ms;
  double stage_ms[8];       /* host clock between the waits of the run: 0 upload + inflate + CRC + segment walk, 1 waiting for
                               the turn, 2 the turn (carry, link), 3 fields / filters / scans, 4 unpack, 5 search, 6 results down */
} svdss_bam_result_t;
int svdss_bam_batch_result(const svdss_bam_batch_t* b, svdss_bam_result_t* out);
/* The same front end (inflate, CRC, record chain, the turn) for `SVDSS call`, which needs whole records of FEW reads:
 * Clusterer::load_batch keeps the primary alignments with mapq >= min_mapq whose read has SFS (clusterer.cpp:108-145),
 * fill_clusters those that overlap a cluster (sam_itr_querys per cluster, :495-545).  A filter names what is kept: records
 * without flags 4 / 256 / 2048, with mapq >= min_mapq, and -- when names and / or regions are given -- whose read name is
 * in `names` (name i = names[name_off[i] .. name_off[i + 1])) or whose alignment [pos, bam_endpos) overlaps one of the
 * regions [reg_beg, reg_end) of its reference (sorted by (tid, beg)); names = NULL: no name test, names given with
 * n_names = 0: the empty set (no record passes by name).  Names are compared by a 64-bit hash: a kept record
 * may rarely be one nobody asked for (the caller looks at the name anyway), a wanted one is never dropped.
 * svdss_bam_select_run takes a batch like svdss_bam_batch_run; the kept records (block_size field first, as in the file)
 * come back in file order at 4-aligned offsets of one page-locked buffer. */
typedef struct svdss_bam_filter svdss_bam_filter_t;
int svdss_bam_filter_create(int32_t device, int32_t min_mapq, int32_t n_ref, const char* names, const int64_t* name_off,
                            int64_t n_names, const int32_t* reg_tid, const int32_t* reg_beg, const int32_t* reg_end,
                            int64_t n_regions, svdss_bam_filter_t** out);
void svdss_bam_filter_free(svdss_bam_filter_t* f);
int svdss_bam_select_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_filter_t* f,
                         int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                         const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                         svdss_bam_batch_t** out);
typedef struct svdss_bam_selection {
  int64_t n_records;        /* records of the batch */
  int64_t n_selected;       /* kept */
  int64_t n_bytes;
  const int64_t* rec_off;   /* n_selected + 1: kept record k begins at bytes + rec_off[k] (its 4-byte block_size, then the record) */
  const uint8_t* bytes;
  double inflate_kernel_ms;
  double stage_ms[8];
  int32_t slim;             /* 1: the records are slim ones (svdss_bam_store_select) */
} svdss_bam_selection_t;
int svdss_bam_batch_selection(const svdss_bam_batch_t* b, svdss_bam_selection_t* out);
/* ONE pass over the file for `SVDSS call`.  Clusterer::run reads the BAM twice: align_and_extend places the SFS of the reads
 * that have any (clusterer.cpp:56-156), fill_clusters fetches, per cluster, the alignments that overlap it (sam_itr_querys,
 * :477-610).  What the second pass looks at of a record is its core, name, CIGAR, bases and HP tag; a svdss_bam_store_t keeps
 * exactly that ("slim" record: block_size | core | name | CIGAR | packed bases | HP as one int32 tag when the record had an
 * integer one -- no qualities, no other tags; ~1/3 of the record) of EVERY record that passes the flag / mapq filters, in
 * HBM, while the first pass runs (svdss_bam_select_store_run = svdss_bam_select_run + the store); the second pass is then a
 * kernel over resident records (svdss_bam_store_select, per stored batch: the slim records that overlap a region of the
 * filter come down, in file order).  With a store the records of the first pass come down slim as well (slim = 1).  A store
 * that would exceed max_bytes stays incomplete (svdss_bam_store_batches): the caller reads the file again, through its
 * index or the device path, as before.  initial_bytes: allocated at once (what the caller expects the store to need: an
 * allocation in the middle of the stream stalls it); the rest in arenas of SVDSS_STORE_ARENA_MB (2,048). */
typedef struct svdss_bam_store svdss_bam_store_t;
int svdss_bam_store_create(int32_t device, int64_t max_bytes, int64_t initial_bytes, svdss_bam_store_t** out);
void svdss_bam_store_free(svdss_bam_store_t* t);
int64_t svdss_bam_store_batches(svdss_bam_store_t* t, int32_t* complete, int64_t* n_records, int64_t* n_bytes);
int svdss_bam_store_reset(svdss_bam_store_t* t);   /* forget what is stored, keep the memory (a file region that runs again) */
int svdss_bam_select_store_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_filter_t* f,
                               svdss_bam_store_t* store, int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                               const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                               svdss_bam_batch_t** out);
/* svdss_bam_store_select applies the filter as svdss_bam_select_run does: a stored record comes down if its name's hash is
 * in the filter's set OR its alignment overlaps a region (either is enough: the caller tests the names exactly).  With a
 * names filter a filled store serves `call`'s FIRST pass as well -- the records of the reads that have SFS, in file order. */
int svdss_bam_store_select(svdss_bam_store_t* t, int64_t seq, const svdss_bam_filter_t* f, svdss_bam_batch_t** out);
/* `SVDSS smooth` on the same front end (csrc/bam_smooth.hip): BGZF blocks in, BGZF blocks out; the inflated records never
 * leave the device.  Stands where smoother.cpp:349-571 stand (loader :498-571 with the filters of :509-537, smooth_read
 * :84-232, rebuild_bam_entry :50-82, the writer :441-494).  A svdss_bam_smooth_t names the reference (svdss_ref_upload:
 * upper-case ASCII), tid_map[t] = chromosome of BAM reference t in it or -1 (records on it are dropped, like every record
 * that is unmapped, secondary, supplementary, below min_mapq or shorter than 2 bases).
 * svdss_bam_smooth_measure: a batch like svdss_bam_batch_run; the kept records' matches / mismatches over their M
 * operations and whether their CIGAR fits read and contig come down (compute_maxaccuracy, smoother.cpp:259-346).
 * svdss_bam_smooth_run: every kept record rewritten (XF 0: smoothed -- equal to the reference except at indels longer than
 * 20 and clips --, 1: mismatch rate above max_mismatch_rate, 2: nothing interesting, 3: CIGAR does not fit; 1-3 keep bases
 * and CIGAR), in file order, as the bytes of a BAM stream cut into BGZF blocks of 0xff00 bytes wherever the batches end:
 * batches take a second turn in file order at which the bytes behind a batch's last full block go to the next one
 * (svdss_bam_stream_set_output_prefix: what precedes batch 0 -- the BAM header of the output).  The blocks of a batch
 * (deflated by csrc/deflate.hip, CRC32 / ISIZE filled in) are in svdss_bam_smoothed_t::bgzf -- in host_out when it is
 * given and large enough (page-locked memory of the caller's, svdss_host_alloc: the writer then needs no copy), else in
 * memory of the batch object; the batch with is_last also holds the stream's short last block; the 28-byte EOF marker is
 * the caller's. */
typedef struct svdss_ref svdss_ref_t;
typedef struct svdss_bam_smooth svdss_bam_smooth_t;
int svdss_bam_smooth_create(const svdss_ref_t* ref, const int32_t* tid_map, int32_t n_ref, int32_t min_mapq,
                            svdss_bam_smooth_t** out);
void svdss_bam_smooth_free(svdss_bam_smooth_t* s);
int svdss_bam_stream_set_output_prefix(svdss_bam_stream_t* s, const uint8_t* bytes, int64_t n);
int svdss_bam_smooth_measure(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_smooth_t* sm,
                             int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                             const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                             svdss_bam_batch_t** out);
int svdss_bam_smooth_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, const svdss_bam_smooth_t* sm,
                         double max_mismatch_rate, uint8_t* host_out, int64_t host_cap, int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                         const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                         svdss_bam_batch_t** out);
typedef struct svdss_bam_smoothed {
  int64_t n_records;              /* records of the batch */
  int64_t n_kept;                 /* of them kept */
  const int64_t* match_mismatch;  /* measure: 2 per kept record */
  const uint8_t* fits;            /* measure: 1 per kept record */
  int64_t out_bytes;              /* run: bytes of the batch's records in the output stream */
  const uint8_t* bgzf;            /* run: the batch's BGZF members, back to back (host memory of the batch object) */
  int64_t bgzf_bytes;
  int64_t n_xf[4];                /* run: records by XF value */
  double inflate_kernel_ms;
  double stage_ms[8];             /* 0-2 as svdss_bam_result_t, 3 filters + CIGAR walk, 4 sizes + records, 5 the output turn, 6 deflate + down,
                                     7 the reads exported for a search, and searched (svdss_bam_smooth_set_search) */
} svdss_bam_smoothed_t;
int svdss_bam_batch_smoothed(const svdss_bam_batch_t* b, svdss_bam_smoothed_t* out);
/* `smooth --write-index` (csrc/bam_smooth.hip, csrc/bam_index_writer.h): svdss_bam_smooth_set_index(sm, min_shift, depth)
 * asks every later svdss_bam_smooth_run on sm for the batch's index fragments (min_shift 0: none, the default; BAI is 14 / 5).
 * They are reduced on the device: one chunk per run of consecutive kept records with the same (tid, bin), one window entry
 * (16 kb at min_shift 14) per window that a record of the batch reaches into first.  Virtual offsets are relative to the
 * batch: (compressed offset from the batch's first member) << 16 | offset in the block; a position at or behind the end of
 * the batch's last member is addressed from the offset right after it (the next member of the output). */
typedef struct svdss_bam_index_chunk {
  int32_t tid;
  uint32_t bin;
  int64_t n_rec;                  /* records of the run */
  uint64_t v_beg, v_end;          /* first record's start, last record's end */
} svdss_bam_index_chunk_t;
typedef struct svdss_bam_index_window {
  int32_t tid;
  int32_t window;                 /* position >> min_shift */
  uint64_t v_beg;                 /* start of the first record of the batch that reaches into the window */
} svdss_bam_index_window_t;
typedef struct svdss_bam_index_frag {
  int64_t n_chunks;
  const svdss_bam_index_chunk_t* chunks;    /* in file order */
  int64_t n_windows;
  const svdss_bam_index_window_t* windows;  /* in file order */
  int32_t unsorted;               /* a kept record starts before the one in front of it (tid, then position) */
  int32_t first_tid, last_tid;    /* the batch's first and last kept record (n_chunks > 0) */
  int64_t first_beg, last_beg;
} svdss_bam_index_frag_t;
int svdss_bam_smooth_set_index(svdss_bam_smooth_t* sm, int32_t min_shift, int32_t depth);
/* `smooth --compress`: every later svdss_bam_smooth_run on sm deflates its BGZF members in this mode (SVDSS_DEFLATE_RUNS,
 * the default, or SVDSS_DEFLATE_LZ; see svdss_bgzf_deflate_mode).  The records, the members' inflated bytes and the index
 * fragments' offsets inside a block do not depend on it; the compressed offsets follow the members' lengths. */
int svdss_bam_smooth_set_deflate(svdss_bam_smooth_t* sm, int32_t mode);
int svdss_bam_batch_index(const svdss_bam_batch_t* b, svdss_bam_index_frag_t* out);
/* ---- the index of the INPUT BAM (`SVDSS bamindex`, `call / run --write-bam-index`; csrc/bam_device.hip, csrc/bam_index_writer.h)
 * Seam: what `samtools index` (htslib's bam_index_build: hts_idx_push per record read by sam_read1) does in a pass of its own
 * in front of run_svdss; here the records are indexed where the device path has them anyway, inflated in HBM.
 * svdss_bam_stream_set_input_index(s, min_shift, depth), before batch 0 (min_shift 0: off, the default; BAI is 14 / 5): every
 * entry point that runs a batch of the stream -- svdss_bam_batch_front / _run, svdss_bam_select_run / _select_store_run,
 * svdss_bam_smooth_measure / _run -- leaves the batch's input-side fragments on the batch object (svdss_bam_batch_input_index).
 * EVERY record that starts in the batch's turn counts, whatever its flag or mapq, and in front of the record gate
 * (svdss_bam_stream_set_regions): tid >= 0 is indexed at [pos, bam_endpos) (a span of 0 counts as 1), tid < 0 is counted.
 * Off, nothing more is launched, allocated or copied; what the entry points return does not depend on the switch.
 * Virtual offsets are relative to the batch's first member: (compressed offset of the member that holds the byte, from the
 * first member's gzip header) << 16 | offset in it.  A position at a member boundary is the start of the next non-empty
 * member; the end of the batch's last byte is comp_bytes << 16 (ends_at_boundary: to be moved to the next non-empty member
 * of the file, or to its EOF marker, by whoever folds the batches).  A record that began in an earlier batch starts where
 * its first byte is: the stream remembers the virtual offset of its carry; such an offset is below the batch's base and
 * wraps as an unsigned number (adding the base << 16 modulo 2^64 gives the file's). */
typedef struct svdss_bam_input_chunk {
  int32_t tid;
  uint32_t bin;
  int64_t n_rec, n_unmapped;      /* records of the run; those of them with flag 4 set */
  uint64_t v_beg, v_end;          /* first record's start, last record's end */
} svdss_bam_input_chunk_t;
typedef struct svdss_bam_input_window {
  int32_t tid;
  int32_t window;                 /* position >> min_shift */
  uint64_t v_beg;                 /* start of the first record of the batch that reaches into the window */
} svdss_bam_input_window_t;
typedef struct svdss_bam_input_frag {
  int32_t on;                     /* 0: the stream's switch was off (everything else is 0) */
  int32_t unsorted;               /* a record starts before the one in front of it (tid, then position; tid < 0 behind all) */
  int64_t n_records, n_no_coor;   /* records that start in this batch's turn; those with tid < 0 */
  int64_t n_chunks;
  const svdss_bam_input_chunk_t* chunks;    /* runs of consecutive indexed records with the same (tid, bin), in file order */
  int64_t n_windows;
  const svdss_bam_input_window_t* windows;  /* in file order */
  int32_t first_tid, last_tid;    /* the first and last record (n_records > 0) */
  int64_t first_beg, last_beg;
  int64_t comp_bytes;             /* compressed length of the batch's members: the next batch's base is this batch's + comp_bytes */
  int64_t first_data;             /* compressed offset of the batch's first non-empty member (-1: it has none) */
  int32_t ends_at_boundary;       /* the last record ends with the batch's last byte */
} svdss_bam_input_frag_t;
int svdss_bam_stream_set_input_index(svdss_bam_stream_t* s, int32_t min_shift, int32_t depth);
int svdss_bam_batch_input_index(const svdss_bam_batch_t* b, svdss_bam_input_frag_t* out);
/* `SVDSS bamindex`: a batch through the front end alone -- blocks up, inflate, CRC, the record chain, the batch's turn and
 * (with the switch on) the index kernels; nothing is filtered, unpacked or copied down but the fragments.  n_records of the
 * batch: svdss_bam_input_frag_t.  Errors as svdss_bam_batch_run ("corrupt record" for fields that do not fit a block_size). */
int svdss_bam_index_run(svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip, int32_t device,
                        int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                        const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                        svdss_bam_batch_t** out);
/* Regions of a file (svdss_bam_stream_region).  svdss_bam_stream_input_seam, after the last batch: *carry_v = the virtual
 * offset of the first byte of the tail, relative to the member right behind the region (has_carry 0: no tail); *head_v = the
 * virtual offset of the first record the chain of an open_start region was started at, relative to the region's first member.
 * A record the seam completes begins at the first and ends at the second.  svdss_bam_stream_set_input_carry, before batch 0
 * of a region that runs again from a known carry: where that carry's first byte is, relative to the region's first member. */
int svdss_bam_stream_input_seam(const svdss_bam_stream_t* s, int32_t* has_carry, int64_t* carry_v, int64_t* head_v);
int svdss_bam_stream_set_input_carry(svdss_bam_stream_t* s, int64_t carry_v);
/* The fold (BamIndexBuilder, csrc/bam_index_writer.h) for callers without C++: fragments in file order, each with the file
 * offset of its batch's first member; finish with the offset of the file's EOF marker (or the file's size where it has none)
 * gives the BAI (csi 0) or CSI bytes, owned by the object.  create: SVDSS_ERANGE for a BAI with a reference longer than
 * 2^29 - 1; finish: SVDSS_EIO where the records are not sorted by coordinate. */
typedef struct svdss_bam_input_indexer svdss_bam_input_indexer_t;
int svdss_bam_input_indexer_create(int32_t n_ref, const int32_t* ref_len, int32_t csi, int32_t* min_shift, int32_t* depth, svdss_bam_input_indexer_t** out);
int svdss_bam_input_indexer_add(svdss_bam_input_indexer_t* ix, const svdss_bam_input_frag_t* f, int64_t base);
int svdss_bam_input_indexer_finish(svdss_bam_input_indexer_t* ix, int64_t end_offset, const uint8_t** bytes, int64_t* n_bytes);
void svdss_bam_input_indexer_free(svdss_bam_input_indexer_t* ix);
/* `smooth --index --sfs` (csrc/bam_smooth.hip): one pass over the original BAM yields what `SVDSS search` would find in the
 * smoothed one.  Seam: ping_pong.cpp:53-128 read the smoothed file back (load_batch_bam :66-104: flag and l_qseq filters,
 * qname, HP, XF, seq_nt16 -> nt6); here those fields are taken from the rebuilt records while they are in HBM.
 *   svdss_bam_smooth_set_search  flags >= 0 (SVDSS_SFS_ASSEMBLE, SVDSS_BAM_PUTATIVE): every later svdss_bam_smooth_run on sm
 *                                also leaves what svdss_bam_batch_front leaves -- names / HP / slots of the kept records with
 *                                a rebuilt l_seq >= 100 on the host (svdss_bam_batch_result; n_short: the shorter ones), the
 *                                searched reads as nt6 in `park` (svdss_bam_batch_parked: group >= 0) or, with park = NULL,
 *                                no room in it or closed, in the batch object (group -1; -2: nothing to search).
 *                                flags = -1, park = NULL: off (the default).
 *   svdss_bam_smooth_search      finishes a batch of group -1 against a resident index, like svdss_bam_batch_search; the
 *                                smoothing run's stage_ms stay, the search is added to stage 7.
 *   svdss_bam_smooth_set_output  write_bam = 0 (`--nobam`): later runs take and pass on the output turn but keep no tail,
 *                                deflate nothing and bring nothing down (bgzf_bytes = 0, no index fragments); 1: the default.
 *   svdss_bam_smooth_set_store   `SVDSS run` (smooth, search and call in one pass over the BAM): every later svdss_bam_smooth_run
 *                                on sm also deposits, under the batch's seq, the slim form of every record of the batch that
 *                                passes `call`'s filters (flags 4 / 256 / 2048 clear, mapq >= min_mapq; clusterer.cpp:118-122)
 *                                -- whether the smoothing keeps the record or not -- byte for byte what
 *                                svdss_bam_select_store_run leaves for the same chunks (one predicate, one export kernel).  A
 *                                store over its limit stays incomplete; the smoothing is unaffected.  store = NULL: off (the
 *                                default).  The store is of sm's device.  svdss_bam_smooth_measure deposits nothing. */
int svdss_bam_smooth_set_search(svdss_bam_smooth_t* sm, int32_t flags, svdss_bam_park_t* park);
int svdss_bam_smooth_set_store(svdss_bam_smooth_t* sm, svdss_bam_store_t* store, int32_t min_mapq);
int svdss_bam_smooth_set_output(svdss_bam_smooth_t* sm, int32_t write_bam);
int svdss_bam_smooth_search(svdss_bam_batch_t* b, const svdss_index_t* ix);
const char* svdss_bam_batch_error(const svdss_bam_batch_t* b);
void svdss_bam_batch_free(svdss_bam_batch_t* b);

/* ---- FASTA / FASTQ records found on the device (csrc/fastx_device.hip) ------------------------------------------
 * Replaces the kseq loop of PingPong::load_batch_fastq (ping_pong.cpp:130-173: kseq_read per record, rb3_char2nt6 per
 * base) for a run of text at once, followed by the search of svdss_sfs_search_batch_device.
 * A svdss_fastx_stream_t is one input being read: it holds the bytes behind a batch's last complete record (the carry,
 * at most carry_cap bytes) and gives the batches their turn in file order; everything else of a batch -- upload,
 * inflate, CRC, names, bases, search -- overlaps with the other batches, each on its own svdss_fastx_batch_t.
 * svdss_fastx_batch_run, batch number seq = 0, 1, 2, ... (every number exactly once, from any thread; is_last on the
 * final one).  The batch's bytes are either BGZF members (n_chunks pieces as for svdss_bam_batch_run, CRC32 checked) or
 * plain text (plain, plain_bytes; n_chunks = 0).  ix = NULL: parse only, on the stream's device (the result then holds
 * the reads); else on the index's device, searched with flags (SVDSS_SFS_ASSEMBLE).
 * The parser delivers a batch in one of two shapes and proves that the host's FastxReader returns the same records:
 * FASTA (first byte '>': no '\r', no NUL, no line beginning with '@') and FASTQ in groups of four lines (first byte
 * '@': no '\r', no NUL; '@' line, a line beginning with neither '>' nor '+', '+' line, a line as long as the second;
 * empty lines only at the end of the stream).  Anything else -- a record longer than carry_cap as well -- is declined:
 * the batch holds the records proved in front of that point and the text from its first unparsed byte on; every later
 * batch of the stream is declined too and holds its text alone (the caller reads on with FastxReader).
 * Errors: SVDSS_EIO with svdss_fastx_batch_error() = "BGZF inflate failed" | "BGZF block CRC mismatch"; once a batch
 * failed every later batch of the stream returns its error. */
typedef struct svdss_fastx_stream svdss_fastx_stream_t;
typedef struct svdss_fastx_batch svdss_fastx_batch_t;
int svdss_fastx_stream_create(int32_t device, int64_t carry_cap, svdss_fastx_stream_t** out);
void svdss_fastx_stream_free(svdss_fastx_stream_t* s);
const char* svdss_fastx_stream_error(const svdss_fastx_stream_t* s);
int svdss_fastx_batch_run(svdss_fastx_stream_t* s, int64_t seq, int32_t is_last, const svdss_index_t* ix,
                          int32_t n_chunks, const uint8_t* const* comp, const int64_t* comp_bytes,
                          const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                          const uint8_t* plain, int64_t plain_bytes, int32_t flags, svdss_fastx_batch_t** out);
/* What the last run of a batch object left on the host (valid until its next run / svdss_fastx_batch_free). */
typedef struct svdss_fastx_result {
  int64_t n_records;        /* records delivered: proved, in file order */
  const int32_t* name_off;  /* n_records + 1: record i is called names[name_off[i] .. name_off[i + 1]) */
  const char* names;
  const int32_t* seq_len;   /* n_records */
  const int64_t* counts;    /* n_records: SFS per record (ix given) */
  const int32_t* qs;        /* total_sfs, record after record */
  const int32_t* len;
  int64_t total_sfs;
  const uint8_t* reads;     /* parse only: the nt6 reads back to back ... */
  const int64_t* offsets;   /* ... read i = reads[offsets[i] .. offsets[i + 1]) */
  int32_t declined;         /* 1: the text from the first unparsed byte on is in `text` */
  int64_t n_text_bytes;     /* carry + this batch's bytes */
  const uint8_t* text;
  int64_t text_bytes;
  double inflate_kernel_ms; /* HIP events */
  double parse_kernel_ms;   /* the parse kernels and their scans, HIP events */
  double stage_ms[8];       /* host clock: 0 upload + inflate + CRC, 1 waiting for the turn, 2 the turn (lines, shape, carry),
                               3 records + names + bases, 5 search, 6 results down */
} svdss_fastx_result_t;
int svdss_fastx_batch_result(const svdss_fastx_batch_t* b, svdss_fastx_result_t* out);
const char* svdss_fastx_batch_error(const svdss_fastx_batch_t* b);
void svdss_fastx_batch_free(svdss_fastx_batch_t* b);
/* bytes per tile of the parse kernels (tests aim at its edges) */
int32_t svdss_fastx_tile_bytes(void);

/* ---- a10: SFS placement ------------------------------------------------------
 * Replaces Clusterer::extend_alignment (clusterer.cpp:159-346) with get_aligned_pairs (bam.cpp:92-134) and
 * get_unique_kmers (clusterer.cpp:351-405) for a batch of alignments: every SFS (qs, len) of a read is mapped to the
 * reference through the read's CIGAR, extended on both sides to the nearest unique clean 7-mer within 100 aligned
 * pairs (ksize 7, flank 100: config.hpp:89-90), and overlapping extended SFS of one read are merged (:314-336).
 * svdss_ref_upload: the chromosome sequences as `call` holds them (upper-case ASCII, chromosomes.cpp:9-27), back to
 * back with off[n_chrom + 1], resident on `device`.
 * Per alignment i: tid[i] (index into the uploaded chromosomes; outside -> nothing placed), pos[i], its BAM CIGAR words
 * cigar[cigar_off[i] .. cigar_off[i+1]) (len << 4 | op), and its SFS sfs_qs/sfs_len[sfs_off[i] .. sfs_off[i+1]) in the
 * order the .sfs file lists them (the reference carries `last_pos` from one to the next, :172-192).
 * Out: out_count[i] merged extended SFS, written at out[5 * (sfs_off[i] + j)]: rs, re, qs, qe (sfs.hpp:52-62 as filled at
 * clusterer.cpp:305-308) and the index (within the read's list) of the first SFS merged into it, whose qname / htag the
 * entry keeps.  stats: SFS counted unplaced, s_unplaced, e_unplaced, unknown (clusterer.cpp:207-226,296). */
typedef struct svdss_ref svdss_ref_t;
int svdss_ref_upload(const uint8_t* seqs, const int64_t* off, int32_t n_chrom, int32_t device, svdss_ref_t** out);
/* the same from one host buffer per chromosome (as load_chromosomes leaves them, chromosomes.cpp:20: a map of strings): no
 * 3 GB copy on the host to put them back to back first */
int svdss_ref_upload_parts(const uint8_t* const* seqs, const int64_t* lens, int32_t n_chrom, int32_t device, svdss_ref_t** out);
void svdss_ref_free(svdss_ref_t* ref);
/* what a svdss_ref_t holds, back on the host (tests): n_chrom, and -- where given -- its n_chrom + 1 offsets and its bytes */
int svdss_ref_read(const svdss_ref_t* ref, int32_t* n_chrom, int64_t* off, uint8_t* seqs);

/* ---- the reference FASTA inflated and parsed on the device (csrc/ref_stream.hip) ---------------------------------
 * Stands where load_chromosomes stands (chromosomes.cpp:9-27: kseq_read per record, toupper per base) and leaves the
 * chromosomes where svdss_ref_upload would put them.  A svdss_ref_stream_t is one FASTA being read in batches numbered in
 * file order (seq = 0, 1, 2, ...: every number exactly once, from any thread; is_last on the final one, which may be
 * empty).  A batch is BGZF members (n_chunks pieces as for svdss_fastx_batch_run, CRC32 checked) or plain text (plain,
 * plain_bytes; n_chunks = 0).  Upload, inflate and CRC of different batches overlap; the parse runs in the batch's turn.
 * The shape: first byte '>', no '\r', no NUL, no line beginning with '@', no header line longer than header_cap bytes
 * ('>' counted, '\n' not), no name twice.  Within it there is a record at every line that begins with '>', named by the
 * bytes behind '>' up to the first blank or tab; its sequence is every other line up to the next header, joined, a-z
 * raised, every other byte kept -- what FastxReader::next and the toupper of load_chromosomes give.  Anything else, a
 * failed inflate and a CRC mismatch (those two also return SVDSS_EIO, from that batch and every later one) DECLINE the
 * stream as a whole: later batches return at once, nothing is delivered, the caller reads the file with the host reader.
 * After the last batch:
 *   svdss_ref_stream_result    the records (or why and where the stream declined) and the counters
 *   svdss_ref_stream_download  one record's bases, from the host copy the batches brought down while later ones ran
 *   svdss_ref_stream_finish    records order[0 .. n) back to back as a svdss_ref_t on `device` (the stream's) -- what
 *                              svdss_ref_upload_parts builds from the same strings -- by device-to-device copies; the
 *                              stream's device memory is freed (once per stream; the host copy stays) */
enum { SVDSS_REF_CR = 1, SVDSS_REF_NUL = 2, SVDSS_REF_AT = 3, SVDSS_REF_NOT_FASTA = 4, SVDSS_REF_DUPLICATE = 5,
       SVDSS_REF_LONG_HEADER = 6, SVDSS_REF_EMPTY = 7, SVDSS_REF_IO = 8, SVDSS_REF_ERROR = 9 };
typedef struct svdss_ref_stream svdss_ref_stream_t;
typedef struct svdss_ref_stream_result {
  int64_t n_records;
  const int64_t* name_off;  /* n_records + 1: record i is called names[name_off[i] .. name_off[i + 1]) */
  const char* names;
  const int64_t* seq_off;   /* n_records + 1: where record i's bases stand in the whole output */
  int32_t declined;         /* 0, or SVDSS_REF_*: nothing above is delivered */
  int64_t declined_at;      /* the byte of the text it was decided at */
  int64_t n_batches;        /* batches that had their turn */
  int64_t text_bytes;
  double inflate_kernel_ms; /* HIP events, summed over the batches */
  double parse_kernel_ms;
} svdss_ref_stream_result_t;
int svdss_ref_stream_create(int32_t device, int64_t header_cap, svdss_ref_stream_t** out);
int svdss_ref_stream_batch(svdss_ref_stream_t* s, int64_t seq, int32_t is_last, int32_t n_chunks, const uint8_t* const* comp,
                           const int64_t* comp_bytes, const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc,
                           const int64_t* n_blocks, const uint8_t* plain, int64_t plain_bytes);
int svdss_ref_stream_result(const svdss_ref_stream_t* s, svdss_ref_stream_result_t* out);
int svdss_ref_stream_download(const svdss_ref_stream_t* s, int64_t rec, uint8_t* dst);
int svdss_ref_stream_finish(svdss_ref_stream_t* s, const int32_t* order, int32_t n, int32_t device, svdss_ref_t** out);
/* the host copy is not needed any more (the caller has its records): its memory goes back; svdss_ref_stream_download fails from here on */
void svdss_ref_stream_drop_host(svdss_ref_stream_t* s);
void svdss_ref_stream_free(svdss_ref_stream_t* s);
const char* svdss_ref_stream_error(const svdss_ref_stream_t* s);
/* bytes per tile of its kernels (tests aim at its edges) */
int32_t svdss_ref_stream_tile_bytes(void);

int svdss_place_sfs_batch(svdss_ref_t* ref, const int32_t* tid, const int32_t* pos, const uint32_t* cigar,
                          const int64_t* cigar_off, const int32_t* sfs_qs, const int32_t* sfs_len, const int64_t* sfs_off,
                          int64_t n_aln, int32_t* out_count, int32_t* out, int64_t stats[4]);

/* ---- smooth: Smoother::smooth_read (smoother.cpp:84-232) for a batch of alignments --------------------------------
 * Per alignment i (all of them eligible and consistent: the caller filters as smoother.cpp:509-537 does and checks that
 * the CIGAR stays inside the chromosome and adds up to l_seq): tid / pos / CIGAR words as for svdss_place_sfs_batch, the
 * packed 4-bit bases at seq4[seq4_off[i]], the qualities at qual[qual_off[i]], l_seq[i].  The kernel walks the CIGAR:
 * M/=/X copy the reference and count matches / mismatches against the read; I and D of at most 20 bases (config.hpp:95)
 * are dropped / filled from the reference, longer ones and soft clips are kept; adjacent M runs merge.  Out, per
 * alignment: the new bases 4-bit packed at out_seq4[cap_off[i] / 2], the new qualities at out_qual[cap_off[i]]
 * (cap_off: caller-chosen even capacities in bases, >= query + reference length of the alignment), the new CIGAR words at
 * out_cigar[cigar_off[i]] with out_ncig[i] of them, out_len[i] bases, out_match_mismatch[2i], [2i+1] (the XF = 1 test is
 * mismatch / match > accuracy, smoother.cpp:213) and out_ignore[i] (nothing interesting: XF = 2, :215). */
int svdss_smooth_batch(svdss_ref_t* ref, const int32_t* tid, const int32_t* pos, const uint32_t* cigar,
                       const int64_t* cigar_off, const uint8_t* seq4, const int64_t* seq4_off, const uint8_t* qual,
                       const int64_t* qual_off, const int32_t* l_seq, const int64_t* cap_off, int64_t n,
                       uint8_t* out_seq4, uint8_t* out_qual, uint32_t* out_cigar, int32_t* out_ncig, int32_t* out_len,
                       int64_t* out_match_mismatch, uint8_t* out_ignore);

/* ---- a15: global dual-affine realignment of consensus to reference --------
 * Replaces ksw_extd2_sse(km=0, qlen, query, tlen, target, m, mat, q, e, q2, e2,
 * w=-1, zdrop=-1, end_bonus=-1, flag=0, &ez) as called at caller.cpp:348-349
 * (ksw2 @HEAD), for a batch of (query = POA consensus, target = reference
 * window) pairs.  Symbols are 0..m-1 (caller.hpp:25-37 _char26_table: ACGT ->
 * 0-3, other -> 4); mat is the m x m substitution matrix (caller.cpp:336-337).
 * Per pair: score = ez.score (VCF `AS`, caller.cpp:351) and the CIGAR as ksw2
 * packs it, len<<4 | op with op 0=M 1=I 2=D (caller.cpp:353-355), gaps
 * left-aligned, from a backtrack at (tlen-1, qlen-1).  Empty query or target:
 * score 0, no CIGAR (ksw2 returns before touching ez). */
typedef struct svdss_aln_batch svdss_aln_batch_t;

int svdss_align_global_batch(const uint8_t* queries, const int64_t* q_off, const uint8_t* targets,
                             const int64_t* t_off, int64_t n_pairs, int32_t m, const int8_t* mat,
                             int32_t gapo, int32_t gape, int32_t gapo2, int32_t gape2, int32_t device,
                             svdss_aln_batch_t** out);
int64_t svdss_aln_batch_npairs(const svdss_aln_batch_t* b);
int64_t svdss_aln_batch_total_cigar(const svdss_aln_batch_t* b);   /* sum of n_cigar */
int64_t svdss_aln_batch_cells(const svdss_aln_batch_t* b);         /* sum of tlen*qlen */
double svdss_aln_batch_kernel_ms(const svdss_aln_batch_t* b);
/* how the last call ran (tests assert the path they were written for): out[0] chunks launched, out[1] pairs laid out
 * with more than one wavefront, out[2] the kernel's wavefronts per workgroup, the largest over the chunks (1, 4 or 8),
 * out[3] chunks run again with one wavefront per pair after a wait that did not end.  All 0 after an empty batch. */
int svdss_aln_batch_launch_info(const svdss_aln_batch_t* b, int64_t out[4]);
/* what the last call computed of its matrices (csrc/aln_band.h; SVDSS_ALIGN_BAND): out[0] wavefront steps executed, out[1]
 * the steps of the full matrices, out[2] pairs run as one band of diagonals, out[3] pairs run as two bands with the gap
 * carried across.  All 0 after an empty batch. */
int svdss_aln_batch_band_info(const svdss_aln_batch_t* b, int64_t out[4]);
/* scores int32[n_pairs], n_cigar int64[n_pairs], cigar uint32[total_cigar] (pairs concatenated) */
int svdss_aln_batch_fetch(const svdss_aln_batch_t* b, int32_t* scores, int64_t* n_cigar, uint32_t* cigar);
void svdss_aln_batch_free(svdss_aln_batch_t* b);

/* ---- a14: partial-order-alignment consensus --------------------------------
 * Replaces Caller::run_poa's abpoa_msa + consensus read-out (caller.cpp:257-308; abPOA
 * v1.5.3: global, convex gap 4/2/24/1, match 2, mismatch 4, no seeding, input order, one
 * heaviest-bundle consensus) for a batch of sub-clusters.  abPOA's source is not available;
 * the algorithm is specified in oracle/svdss_oracle_poa.c (tolerance vs abPOA: DESIGN.md).
 * seqs: symbols 0..4 (caller.hpp:25-37) of all reads concatenated, seq_off[n_seqs+1];
 * cluster c owns reads cluster_off[c] .. cluster_off[c+1]-1, aligned in that order.
 * Result per cluster: consensus symbols 0..4 ("ACGTN"[b], caller.cpp:297); empty for a
 * cluster without reads. */
typedef struct svdss_poa_batch svdss_poa_batch_t;

int svdss_poa_consensus_batch(const uint8_t* seqs, const int64_t* seq_off, const int64_t* cluster_off,
                              int64_t n_clusters, int32_t device, svdss_poa_batch_t** out);
int64_t svdss_poa_batch_nclusters(const svdss_poa_batch_t* b);
int64_t svdss_poa_batch_total(const svdss_poa_batch_t* b);     /* sum of consensus lengths */
int64_t svdss_poa_batch_cells(const svdss_poa_batch_t* b);     /* DP cells computed */
double svdss_poa_batch_kernel_ms(const svdss_poa_batch_t* b);
/* sub-clusters the LDS-resident kernel handed to the HBM kernel (graph too large for LDS, a node with
 * more than 8 predecessors, or the full-matrix fallback of the band) */
int64_t svdss_poa_batch_hbm(const svdss_poa_batch_t* b);
/* sub-clusters the first stage (several sub-clusters per wavefront, csrc/poa_quad.hip) handed on to the
 * one-wavefront-per-sub-cluster rounds: a row wider than its lanes, a node with more than 7 predecessors, a band that
 * lost the sink, a graph beyond its first allocation */
int64_t svdss_poa_batch_quad_back(const svdss_poa_batch_t* b);
/* developer check of the cross-lane primitives of csrc/poa_quad_core.h (DPP shifts / scans / rotations, permutes,
 * ballots) on the device: in = 64 values, out = 3 x 64 x 12 values (group widths 16, 32, 64); tests/test_poa_quad_gpu.py
 * holds them against the definitions the CPU wave emulator of the tests uses */
int svdss_poa_quad_selftest(const int32_t* in, int32_t* out, int32_t device);
int svdss_poa_batch_fetch(const svdss_poa_batch_t* b, int64_t* cons_len, uint8_t* cons);
void svdss_poa_batch_free(svdss_poa_batch_t* b);

/* ---- a17: rapidfuzz::fuzz::ratio(a, b) (rapidfuzz-cpp v1.10.4) -----------
 * as called at caller.cpp:456,458 on the REF/ALT alleles of adjacent SVs:
 * 100 * (1 - (|a|+|b| - 2 LCS(a,b)) / (|a|+|b|)), 100 for two empty strings.
 * a/b: concatenated byte strings with offsets[n_pairs+1].  lcs_out may be NULL. */
int svdss_indel_ratio_batch(const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off,
                            int64_t n_pairs, int32_t device, double* ratio_out, int64_t* lcs_out);
/* the kernel the calling thread's last non-empty svdss_indel_ratio_batch launched: 0 bit-parallel, 1 anti-diagonals
 * in LDS, 2 anti-diagonals in HBM, -1 none yet */
int32_t svdss_indel_ratio_last_kernel(void);

/* ---- the streams of the call side ------------------------------------------
 * svdss_poa_consensus_batch, svdss_align_global_batch and svdss_indel_ratio_batch (the seam: Caller::run_poa, the ksw2
 * realignment and the chain filter of caller.cpp, a14 / a15 / a17 above) each run on ONE stream, leased for the call
 * from a process-wide pool (csrc/call_streams.h).  What the pool did so far:
 * out[0] streams of `device` (leased or idle), out[1] streams created since load (all devices), out[2] first-stage POA
 * launches that held both whole-wavefront variants (SVDSS_POA_MERGE=0: none), out[3] leases borrowed for launches that
 * ran side by side.  SVDSS_EINVAL for a null `out` or a device that is negative or beyond the pool's 64. */
int svdss_call_side_stat(int32_t device, int64_t out[4]);

/* ---- plain gzip inflated on the device, chunk-parallel (csrc/gzip_stream.hip, gzip_stream.h) -------------------------
 * ONE deflate stream (what gzip writes, not BGZF) inflated in parallel: the compressed bytes of a window are cut into
 * chunks of chunk_bytes, a block start is searched in every chunk, every chunk is decoded from its start with references
 * into the unknown 32 KB in front of it kept as symbols, and the symbols are resolved chunk after chunk.
 * A svdss_gzip_stream_t is one file being read.  svdss_gzip_stream_run takes the next window: comp[0] is the byte the
 * stream stands in (the first byte of the file at first; afterwards the byte *consumed bytes further on, every time),
 * is_last says that comp reaches the end of the file.  It inflates as far as whole deflate blocks lie inside the window,
 * at most to the end of the current member, whose CRC32 and ISIZE it checks.  A run that neither consumes nor delivers
 * anything and neither ends nor declines needs more bytes in its window.
 * The unit DECLINES what it cannot do (svdss_gzip_result_t.declined, a SVDSS_GZIP_DECLINE_* reason): the run consumes
 * what it could and the caller reads on from the carried state (byte position, bit, the 32 KB in front of it, running
 * CRC32 and count) with zlib: svdss_gzip_stream_host_tail does that for bytes in memory (csrc/gzip_stream.h: GzHostTail).
 * Errors: SVDSS_EIO with svdss_gzip_stream_error() = what is wrong with the stream (a trailer that does not fit, a match
 * that reaches in front of its member). */
typedef struct svdss_gzip_stream svdss_gzip_stream_t;
#define SVDSS_GZIP_DECLINE_HEADER 1      /* the first bytes are not a gzip member header */
#define SVDSS_GZIP_DECLINE_NO_START 2    /* no chunk of the window holds a dynamic block start: nothing to do in parallel */
#define SVDSS_GZIP_DECLINE_NO_ADVANCE 3  /* not one whole block inside the window */
#define SVDSS_GZIP_DECLINE_DAMAGED 4     /* an invalid code at the stream's position */
#define SVDSS_GZIP_DECLINE_TRAILING 5    /* bytes behind a member that are not a gzip member header */
typedef struct svdss_gzip_result {
  const uint8_t* text;        /* what the last run (or host_tail) inflated: page-locked host memory */
  const uint8_t* d_text;      /* ... and the same bytes on the device (NULL after host_tail) */
  int64_t text_bytes;
  /* counters over all runs so far */
  int64_t windows;            /* runs that inflated something */
  int64_t n_chunks;           /* chunks the chain covered */
  int64_t chunks_on_chain;    /* ... decoded from a start of their own */
  int64_t chunks_merged;      /* ... without a start: decoded by the chunk before them */
  int64_t false_starts;       /* ... with a start that no block end met */
  int64_t members_finished;
  int64_t device_bytes;       /* text inflated on the device */
  int32_t ended;              /* the file's last member is finished and nothing follows */
  int32_t declined;           /* 0, or why the host takes over */
  /* the carried state: where the stream stands */
  int64_t byte_pos;           /* of the file */
  int32_t bit;                /* 0..7 in that byte */
  int32_t in_member;          /* 1: inside a deflate stream; 0: at a member header */
  int32_t want_trailer;       /* 1: at a member's CRC32 / ISIZE */
  uint32_t crc;               /* of the member's text so far */
  uint64_t count;             /* bytes of it */
  const uint8_t* dict;        /* the dict_len bytes of text in front of the position (at most 32768) */
  int32_t dict_len;
  double find_ms, measure_ms, decode_ms, resolve_ms;   /* HIP-event time of the kernels, summed over all runs */
} svdss_gzip_result_t;
int svdss_gzip_stream_create(int32_t device, int64_t chunk_bytes, svdss_gzip_stream_t** out);
int svdss_gzip_stream_run(svdss_gzip_stream_t* s, const uint8_t* comp, int64_t comp_bytes, int32_t is_last, int64_t* consumed);
int svdss_gzip_stream_result(const svdss_gzip_stream_t* s, svdss_gzip_result_t* out);
/* comp: the file from byte_pos to its end.  The text is svdss_gzip_result_t.text afterwards. */
int svdss_gzip_stream_host_tail(svdss_gzip_stream_t* s, const uint8_t* comp, int64_t comp_bytes);
const char* svdss_gzip_stream_error(const svdss_gzip_stream_t* s);
void svdss_gzip_stream_free(svdss_gzip_stream_t* s);

#ifdef __cplusplus
}
#endif
#endif /* SVDSS_HIP_H */
