// input.hip -- translation unit of the input readers: the Themisto reader on the host and on the device, the subset of a
// resident alignment (msw_alignment_subset), gzip / BGZF inflation,
// --read-likelihood files and the FASTQ reader, with their C ABI entries.
#include "host_api.hpp"

#include "reader_kernels.hpp"
#include "subset_kernels.hpp"
#include "inflate_kernels.hpp"
#include "inflate_member_kernels.hpp"
#include "likelihood_text_kernels.hpp"
#include "fastq_host.hpp"
#include "fastq_kernels.hpp"

MSW_UNIT_WARM(input)

void msw::host::lik_gather_launch(hipStream_t st, const double *src, const uint64_t *idx, uint32_t n, double *out) {
  hipLaunchKernelGGL(k_lik_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, idx, n, out);
}

#include "host_alignment.inc"
#include "host_reader.inc"
#include "host_subset.inc"
#include "host_inflate.inc"
#include "host_inflate_members.inc"
#include "host_likelihood_file.inc"
#include "host_fastq.inc"

extern "C" {

int msw_core_set_dense_logl_file(msw_handle h, const char *path, size_t n_groups, msw_likfile_info *info) {
  return guarded(h, [&] {
    if (!path) throw Fail("msw_core_set_dense_logl_file: null path");
    set_dense_file_impl(h, path, nullptr, 0, n_groups, info);
  });
}

int msw_core_set_dense_logl_text(msw_handle h, const char *text, size_t n, size_t n_groups, msw_likfile_info *info) {
  return guarded(h, [&] { set_dense_file_impl(h, nullptr, text, n, n_groups, info); });
}

int msw_core_likfile_counts(msw_handle h, uint64_t *counts_out, size_t n_ecs) {
  return guarded(h, [&] { likfile_counts_impl(h, counts_out, n_ecs); });
}

int msw_core_trim(msw_handle h) {
  return guarded(h, [&] {
    MSW_HIP(hipStreamSynchronize(h->stream));
    h->reader_pool.trim();
    h->text.release_device();  // (the pinned text of the last msw_core_text_block stays valid)
    h->gz.release_device();
    h->sparse.drop();  // (msw_core_sparse_probs_begin's selection: device memory throughout)
  });
}

int msw_alignment_read_device(msw_handle h, const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode,
                              msw_alignment_t *out) {
  if (out) *out = nullptr;
  const int rc = guarded(h, [&] {
    check_reader_args(paths, out, n_paths, n_targets, merge_mode);
    std::unique_ptr<msw_alignment> a(new msw_alignment);
    a->device = h->device;
    MSW_HIP(hipStreamSynchronize(h->stream));
    h->reader_pool.recycle();  // (blocks the previous read handed back: nothing of it is in flight any more)
    ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
    cx.inf = &h->inf;
    h->inf.last.clear();
    bool fits = true;
    {  // ~5 bytes of device memory per byte of text (measured: 10 GB at cfg3's 2.09 GB, 45 GB at 9.5 GB): a text that
       // would not fit beside what the device already holds goes to the host reader
      uint64_t text = 0;
      for (size_t i = 0; i < n_paths; ++i) {
        struct stat sb;
        if (paths[i] && stat(paths[i], &sb) == 0) text += (uint64_t)sb.st_size * (path_is_gzip(paths[i]) ? 8u : 1u);
      }
      size_t free_b = 0, total_b = 0;
      MSW_HIP(hipMemGetInfo(&free_b, &total_b));
      // (what earlier reads left idle on the handle counts as room; when it would be needed as FRESH memory -- a text of
      // another size class -- it goes back to the device first)
      const uint64_t need = 6 * text + (1ull << 30);
      if (need > (uint64_t)free_b && h->reader_pool.idle_bytes()) {
        h->reader_pool.trim();
        MSW_HIP(hipMemGetInfo(&free_b, &total_b));
      }
      fits = need <= (uint64_t)free_b + h->reader_pool.idle_bytes();
      if (getenv("MSWEEP_READER_FORCE_HOST")) fits = false;  // developer switch (tests): the host reader behind this entry
    }
    try {
      if (!fits) throw ReaderFallback{};
      try {
        read_alignment_device(paths, n_paths, n_targets, merge_mode, cx, *a);
      } catch (const HipError &ex) {
        if (!strstr(ex.what(), "out of memory")) throw;
        (void)hipGetLastError();
        throw ReaderFallback{};
      }
    } catch (const ReaderFallback &) {
      // text the kernels do not judge: the host reader's outcome -- a result or the reference's message -- stands
      msw_alignment_t host = nullptr;
      if (msw_alignment_read(paths, n_paths, n_targets, merge_mode, &host) != 0) throw Fail(msw_alignment_last_error());
      *out = host;
      return;
    }
    *out = a.release();
  });
  if (rc != 0 && h) g_aln_error = msw_last_error(h);
  return rc;
}

// ---- gzip input inflated on the device: the test and diagnostic entry, and the report of the last read --------------------
int msw_core_inflate_gzip(msw_handle h, const uint8_t *gz, size_t n, size_t chunk_bytes, const uint8_t **text_out, size_t *len_out,
                          msw_inflate_info *info) {
  return guarded(h, [&] { inflate_gzip_impl(h, gz, n, chunk_bytes, text_out, len_out, info); });
}

int msw_alignment_last_inflate(msw_handle h, msw_inflate_info *info, size_t max_files, size_t *n_files) {
  return guarded(h, [&] { last_inflate_impl(h, info, max_files, n_files); });
}

// ---- --extract-reads: the records of a FASTQ file by read id (host_fastq.inc) ------------------------------------------------
int msw_fastq_open(msw_handle h, const char *path, msw_fastq_t *out, msw_fastq_info *info) {
  return guarded(h, [&] { fastq_open_impl(h, path, out, info); });
}

int msw_fastq_select(msw_handle h, msw_fastq_t fq, const uint32_t *ids, size_t n, uint64_t *n_selected_out, uint64_t *bytes_out) {
  return guarded(h, [&] { fastq_select_impl(h, fq, ids, n, n_selected_out, bytes_out); });
}

int msw_fastq_next(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out) {
  return guarded(h, [&] { fastq_next_impl(h, fq, max_bytes, false, out, len_out, nullptr); });
}

int msw_fastq_next_gzip(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out, size_t *text_len_out) {
  return guarded(h, [&] { fastq_next_impl(h, fq, max_bytes, true, out, len_out, text_len_out); });
}

int msw_fastq_last_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->fastq.kernel_ms;
    if (bytes_out) *bytes_out = h->fastq.bytes;
  });
}

void msw_fastq_close(msw_fastq_t fq) { fastq_close_impl(fq); }

}  // extern "C"
