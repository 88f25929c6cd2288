// ref_loader.h -- the reference FASTA read on the GPU (csrc/ref_stream.hip), beside load_chromosomes (fastx_reader.h):
// the file is cut into batches by FastxBatcher (fastx_device.h), a few feeding threads hand them to the stream, the host
// copy comes back record by record, and the stream is kept so that the chromosomes the BAM header names can be put back
// to back in HBM by device-to-device copies (svdss_ref_stream_finish) instead of going up again.
//
// Used when there is a GPU, the file is BGZF, SVDSS_FASTA_SERIAL is unset and SVDSS_REF_DEVICE is not 0
// (SVDSS_REF_DEVICE=2: also plain files, in slabs -- a developer setting).  Whenever it returns false -- not eligible, or
// the stream declined -- nothing has been delivered and the caller reads the file as before.
#pragma once
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/svdss_hip.h"
#include "fastx_device.h"
#include "fastx_reader.h"
#include "host_common.h"

// what the device loader leaves behind: the finished stream, its output still in HBM (null: the host loaders read the
// file, or resident() took the output)
struct RefOnDevice {
  svdss_ref_stream_t* stream = nullptr;
  std::unordered_map<std::string, int32_t> record_of;
  RefOnDevice() = default;
  RefOnDevice(const RefOnDevice&) = delete;
  RefOnDevice& operator=(const RefOnDevice&) = delete;
  ~RefOnDevice() { drop(); }
  void drop() { if (stream) svdss_ref_stream_free(stream); stream = nullptr; record_of.clear(); }
};

inline const char* ref_decline_reason(int32_t why) {
  static const char* const what[] = {"", "a carriage return", "a NUL byte", "a line that begins with '@'", "the first byte is not '>'",
                                     "a name occurs twice", "a header line longer than 64 KB", "the file is empty", "a BGZF member that does not inflate to its CRC",
                                     "an error on the device"};
  return why >= 0 && why < 10 ? what[why] : "";
}

// names and upper-cased sequences in FASTA order, as load_fasta_mapped(upper = true) leaves them; `keep` (may be null)
// takes the stream.  `tag`: the command's log tag for the --verbose lines.
inline bool load_reference_device(const std::string& path, int threads, bool serial, bool verbose, const char* tag, std::vector<std::string>& names,
                                  std::vector<std::string>& seqs, RefOnDevice* keep) {
  const int mode = (int)env_from("SVDSS_REF_DEVICE", 0, 1);
  if (mode == 0 || serial || svdss_device_count() <= 0) return false;
  const FastxKind kind = fastx_device_kind(path);
  if (kind == FastxKind::None) {
    uint8_t h[2] = {0, 0};
    FILE* f = fopen(path.c_str(), "rb");
    const bool gz = f && fread(h, 1, 2, f) == 2 && h[0] == 0x1f && h[1] == 0x8b;
    if (f) fclose(f);
    if (gz && verbose) fprintf(stderr, "[%s] reference: plain gzip is read by one thread; bgzip it to have it read on the GPU\n", tag);
    return false;
  }
  if (kind == FastxKind::Plain && mode < 2) return false;
  const int64_t batch_bytes = getenv("SVDSS_REF_BATCH_KB") ? env_from("SVDSS_REF_BATCH_KB", 1, 1) << 10 : env_from("SVDSS_REF_BATCH_MB", 1, 64) << 20;
  const size_t slab_bytes = (size_t)env_from("SVDSS_BAM_SLAB_KB", 64, 16 << 10) << 10;
  const int loaders = (int)env_raised("SVDSS_BAM_LOADERS", 1, 8);
  const int feeders = (int)env_raised("SVDSS_REF_FEEDERS", 1, 4);
  const size_t per_batch = (size_t)batch_bytes / slab_bytes + 2;
  FastxBatcher batcher(path, kind, batch_bytes, slab_bytes, loaders, (size_t)loaders + ((size_t)feeders + 3) * per_batch);
  if (!batcher.ok()) return false;
  svdss_ref_stream_t* stream = nullptr;
  if (svdss_ref_stream_create(0, 64 << 10, &stream) != SVDSS_OK) return false;
  std::atomic<int> failed(0);
  auto feed = [&] {
    std::vector<uint8_t> slab;
    FILE* f = kind == FastxKind::Plain ? fopen(path.c_str(), "rb") : nullptr;
    FastxJob job;
    while (!failed.load() && batcher.next(job)) {
      if (kind == FastxKind::Plain) {
        slab.resize((size_t)job.plain_bytes);
        size_t got = 0;
        while (f && got < slab.size()) {
          const ssize_t k = pread(fileno(f), slab.data() + got, slab.size() - got, (off_t)(job.plain_off + (int64_t)got));
          if (k <= 0) break;
          got += (size_t)k;
        }
        if (got < slab.size()) { failed = 1; break; }
      }
      if (svdss_ref_stream_batch(stream, job.seq, job.last ? 1 : 0, (int32_t)job.comp.size(), job.comp.data(), job.comp_bytes.data(), job.blocks.data(),
                                 job.crc.data(), job.n_blocks.data(), slab.data(), job.plain_bytes) != SVDSS_OK)
        failed = 1;
    }
    if (f) fclose(f);
  };
  {
    std::vector<std::thread> th;
    for (int k = 1; k < feeders; ++k) th.emplace_back(feed);
    feed();
    for (std::thread& x : th) x.join();
  }
  svdss_ref_stream_result_t r;
  const bool have = svdss_ref_stream_result(stream, &r) == SVDSS_OK;
  if (failed.load() || !batcher.error().empty() || !have || r.declined) {
    if (verbose) {
      const std::string why = have && r.declined ? std::string(ref_decline_reason(r.declined)) + " at byte " + std::to_string(r.declined_at)
                                                 : batcher.error().empty() ? std::string("the file could not be read") : batcher.error();
      fprintf(stderr, "[%s] reference: the device loader declined (%s): the host reader reads the file\n", tag, why.c_str());
    }
    svdss_ref_stream_free(stream);
    return false;
  }
  // the host copy, record by record (a few threads: every record is a memcpy out of the batches' buffers)
  const size_t R = (size_t)r.n_records;
  std::vector<std::string> nm(R), sq(R);
  for (size_t i = 0; i < R; ++i) nm[i].assign(r.names + r.name_off[i], (size_t)(r.name_off[i + 1] - r.name_off[i]));
  {
    std::atomic<size_t> next(0);
    std::atomic<int> bad(0);
    auto work = [&] {
      for (size_t i = next.fetch_add(1); i < R; i = next.fetch_add(1)) {
        sq[i].resize((size_t)(r.seq_off[i + 1] - r.seq_off[i]));
        if (svdss_ref_stream_download(stream, (int64_t)i, (uint8_t*)&sq[i][0]) != SVDSS_OK) bad = 1;
      }
    };
    std::vector<std::thread> th;
    for (int k = 1; k < std::max(1, std::min(threads, 8)); ++k) th.emplace_back(work);
    work();
    for (std::thread& x : th) x.join();
    if (bad.load()) { svdss_ref_stream_free(stream); return false; }
  }
  if (verbose)
    fprintf(stderr, "[%s] reference: %lld batches on the device, %zu records, %lld bases (inflate kernels %.3f ms, parse kernels %.3f ms)\n", tag,
            (long long)r.n_batches, R, (long long)r.seq_off[R], r.inflate_kernel_ms, r.parse_kernel_ms);
  svdss_ref_stream_drop_host(stream);
  if (keep) {
    keep->drop();
    keep->stream = stream;
    for (size_t i = 0; i < R; ++i) keep->record_of[nm[i]] = (int32_t)i;
  } else {
    svdss_ref_stream_free(stream);
  }
  names.swap(nm);
  seqs.swap(sq);
  return true;
}

// load_chromosomes (fastx_reader.h) with the device loader tried first
inline bool load_chromosomes(const std::string& path, int threads, bool serial, bool verbose, const char* tag, std::vector<std::string>& names,
                             std::unordered_map<std::string, std::string>& seqs, RefOnDevice* keep) {
  std::vector<std::string> nm, sq;
  if (load_reference_device(path, threads, serial, verbose, tag, nm, sq, keep)) {
    for (size_t i = 0; i < nm.size(); ++i) seqs[nm[i]] = std::move(sq[i]);
    names.insert(names.end(), nm.begin(), nm.end());
    return true;
  }
  return load_chromosomes(path, threads, serial, names, seqs);
}

// upload_chromosomes (host_common.h) on GPU 0, out of the stream's output where the device loader left it: the same
// chromosomes in the same order with the same tid_map, by device-to-device copies
inline int resident_chromosomes(RefOnDevice* dev, const std::vector<std::string>& ref_names, const std::unordered_map<std::string, std::string>& seqs,
                                std::vector<int32_t>& tid_map, svdss_ref_t** dref) {
  if (!dev || !dev->stream) return upload_chromosomes(ref_names, seqs, 0, tid_map, dref);
  std::vector<int32_t> order;
  for (const size_t t : header_order(ref_names, [&](const std::string& n) { return dev->record_of.count(n) > 0; }, tid_map)) order.push_back(dev->record_of[ref_names[t]]);
  const int rc = svdss_ref_stream_finish(dev->stream, order.data(), (int32_t)order.size(), 0, dref);
  dev->drop();
  return rc;
}
