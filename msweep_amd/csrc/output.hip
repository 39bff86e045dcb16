// output.hip -- translation unit of the text (dense and sparse) and gzip outputs, with their C ABI entries; k_gz_crc, which the inflate path of
// input.hip needs too, is owned here (host_gzip.inc gz_crc_launch).
#include "host_api.hpp"

#include "text_kernels.hpp"
#include "deflate_kernels.hpp"
#include "sparse_probs_kernels.hpp"

MSW_UNIT_WARM(output)

#include "host_text.inc"
#include "host_gzip.inc"
#include "host_sparse_probs.inc"

extern "C" {

int msw_core_text_block(msw_handle h, int what, size_t ec_begin, size_t ec_end, const uint64_t *line_prefix,
                        size_t n_zero_cols, const char **text_out, size_t *len_out, size_t *n_host_cells_out) {
  return guarded(h, [&] { text_block_impl(h, what, ec_begin, ec_end, line_prefix, n_zero_cols, text_out, len_out, n_host_cells_out); });
}

int msw_core_format_g6(msw_handle h, const double *x, size_t n, const char **text_out, size_t *len_out, size_t *n_host_out) {
  return guarded(h, [&] { format_g6_impl(h, x, n, text_out, len_out, n_host_out); });
}

// ---- --compress z (src/OutfileDesignator.cpp:30-37) -----------------------------------------------------------------------
int msw_core_gzip_begin(msw_handle h, int level, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_begin_impl(h, level, out, len_out); });
}

int msw_core_text_block_gzip(msw_handle h, int what, size_t ec_begin, size_t ec_end, const uint64_t *line_prefix, size_t n_zero_cols,
                             const char **out, size_t *len_out, size_t *n_host_cells_out, size_t *text_len_out) {
  return guarded(h, [&] { text_block_gzip_impl(h, what, ec_begin, ec_end, line_prefix, n_zero_cols, out, len_out, n_host_cells_out, text_len_out); });
}

int msw_core_gzip_append(msw_handle h, const char *bytes, size_t n, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_append_impl(h, bytes, n, out, len_out); });
}

int msw_core_gzip_end(msw_handle h, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_end_impl(h, out, len_out); });
}

int msw_core_last_gzip_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_in_out, uint64_t *bytes_out_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->gz.kernel_ms;
    if (bytes_in_out) *bytes_in_out = h->gz.isize;
    if (bytes_out_out) *bytes_out_out = h->gz.bytes_out;
  });
}

int msw_core_last_text_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->text.kernel_ms;
    if (bytes_out) *bytes_out = h->text.bytes;
  });
}

// ---- --write-read-probs: the probabilities at or above a threshold, one line per cell -------------------------
int msw_core_sparse_probs_begin(msw_handle h, struct msw_alignment *a, double threshold, uint64_t *n_rows_out, double *log_thr_out) {
  return guarded(h, [&] { sparse_probs_begin_impl(h, a, threshold, n_rows_out, log_thr_out); });
}

int msw_core_sparse_probs_next(msw_handle h, size_t max_bytes, const char **text_out, size_t *len_out, uint64_t *rows_done_out,
                               uint64_t *n_cells_out, size_t *n_host_cells_out) {
  return guarded(h, [&] { sparse_probs_next_impl(h, max_bytes, false, text_out, len_out, rows_done_out, n_cells_out, n_host_cells_out, nullptr); });
}

int msw_core_sparse_probs_next_gzip(msw_handle h, size_t max_bytes, const char **out, size_t *len_out, uint64_t *rows_done_out,
                                    size_t *text_len_out) {
  return guarded(h, [&] { sparse_probs_next_impl(h, max_bytes, true, out, len_out, rows_done_out, nullptr, nullptr, text_len_out); });
}

int msw_core_last_sparse_probs_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out, uint64_t *cells_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->sparse.kernel_ms;
    if (bytes_out) *bytes_out = h->sparse.bytes;
    if (cells_out) *cells_out = h->sparse.n_cells;
  });
}

}  // extern "C"
