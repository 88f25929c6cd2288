// bamindex_host.cpp -- `SVDSS bamindex --bam BAM [-o FILE]`: the BAI / CSI index of the BAM the chain is given, what
// `samtools index BAM` writes in front of run_svdss -- one pass over the file through the device path's front end (loaders,
// inflate, record chain) and the index kernels (csrc/bam_device.hip, svdss_bam_index_run), folded by InputIndexFold
// (bam_input_index.h).  --gpus N: the file's regions, one per GPU (ShardedBamSelect).  SVDSS_BAM_DEVICE=0: the host reader.
#define SVDSS_LOG_TAG "bamindex"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "host_common.h"
#include "host_knobs.h"
#include "call_host.h"
#include "bam_input_index.h"

int main_bamindex(const CallOptions& o) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string& out = o.write_bam_index;
  const bool host_asked = env_switch("SVDSS_BAM_DEVICE") == 0;
  // (no GPU and no SVDSS_BAM_DEVICE=0: the command fails rather than quietly running the host reader)
  if (!host_asked && svdss_device_count() <= 0)
    die("no GPU found: SVDSS bamindex indexes the records on the GPU (SVDSS_BAM_DEVICE=0 runs the host reader instead)");
  std::vector<int32_t> lens;
  std::string err;
  if (!bam_header_lengths(o.bam, lens, err)) die("cannot read " + o.bam + ": " + err);
  InputIndexFold fold;
  if (!fold.open(out, lens, "bamindex -o", err)) die(err);
  uint64_t comp_bytes = 0;
  if (host_asked) {
    if (!index_bam_on_host(o.bam, fold, comp_bytes, err)) die("error reading " + o.bam + ": " + err);
  } else {
    int32_t n_ref = 0;
    int64_t skip = 0;
    if (!bam_header_probe(o.bam, n_ref, skip, err, nullptr)) die("cannot read " + o.bam + ": " + err);
    const CallKnobs knobs;
    const int n_dev = std::max(1, svdss_device_count());
    const std::vector<size_t> cuts = plan_bam_regions(o.bam, effective_gpus(o.gpus), skip);
    struct Out { InputFragCopy ix; };
    ShardedBamSelect<Out>::Hooks hooks;
    hooks.run = [n_dev](size_t g, bool) {
      const int32_t dev = (int32_t)(g % (size_t)n_dev);
      return BamRunFn([dev](svdss_bam_stream_t* s, int64_t seq, int32_t is_last, int64_t skip_, size_t, int32_t n_chunks, const uint8_t* const* comp,
                            const int64_t* comp_bytes_, const svdss_bgzf_block_t* const* blocks, const uint32_t* const* crc, const int64_t* n_blocks,
                            svdss_bam_batch_t** batch) {
        return svdss_bam_index_run(s, seq, is_last, skip_, dev, n_chunks, comp, comp_bytes_, blocks, crc, n_blocks, batch);
      });
    };
    hooks.collect = [](size_t g, bool seam) {
      return ShardedBamSelect<Out>::CollectFn([g, seam](const svdss_bam_batch_t* batch, uint64_t) {
        std::unique_ptr<Out> r(new Out);
        r->ix.take(batch, g, seam);
        return r;
      });
    };
    ShardedBamSelect<Out> sel(o.bam, hooks, n_ref, skip, knobs.feeders, knobs.batch_bytes, cuts, 64, std::vector<BgzfScanner*>(), false, fold.shift(),
                              fold.depth());
    while (std::unique_ptr<Out> b = sel.next()) {
      if (!b->ix.seam) comp_bytes += (uint64_t)b->ix.f.comp_bytes;
      fold.add(b->ix, sel);
    }
    if (sel.failure().failed()) die("error reading " + o.bam + ": " + sel.error());
    if (o.verbose)
      fprintf(stderr, "[bamindex] %zu region(s), %lld seam(s), %lld region(s) run again\n", sel.n_regions(), (long long)sel.seams_run(),
              (long long)sel.regions_run_again());
  }
  if (!fold.finish(o.bam, err)) die(err);
  if (o.verbose)
    fprintf(stderr, "[bamindex] %llu records (%llu without a reference), %llu chunks, %llu windows, %llu compressed bytes read, %.3f s (%s)\n",
            (unsigned long long)fold.records(), (unsigned long long)fold.builder()->n_no_coor(), (unsigned long long)fold.builder()->n_chunks(),
            (unsigned long long)fold.builder()->n_windows(), (unsigned long long)comp_bytes,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), host_asked ? "host reader" : "device path");
  logmsg("info", "index of " + o.bam + " written to " + out);
  return 0;
}
