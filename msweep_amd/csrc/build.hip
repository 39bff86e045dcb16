// build.hip -- translation unit of the likelihood build: layout planning, upload and packing, the device build, the dense
// re-expression, gamma, the bin pass (bin_kernels.hpp builds on gamma_kernels.hpp) and the assign pass with its table
// (assign_kernels.hpp builds on bin_kernels.hpp), with their C ABI entries.
#include "host_api.hpp"

#include "sweep_kernels.hpp"
#include "likelihood_kernels.hpp"
#include "pack_kernels.hpp"
#include "compress_kernels.hpp"
#include "gamma_kernels.hpp"
#include "bin_kernels.hpp"
#include "assign_kernels.hpp"

MSW_UNIT_WARM(build)

#include "host_layout.inc"
#include "host_likelihood.inc"
#include "host_pack.inc"
#include "host_build.inc"
#include "host_compress.inc"
#include "host_bin.inc"
#include "host_assign.inc"

extern "C" {

int msw_core_set_dense_logl(msw_handle h, const double *L, size_t n_groups, size_t n_ecs, size_t ld) {
  return guarded(h, [&] { set_dense_impl(h, L, n_groups, n_ecs, ld); });
}

int msw_core_set_csr(msw_handle h, const uint64_t *rowptr, const uint32_t *grp, const uint32_t *cnt,
                     const double *lut, size_t lut_ld, double logzi, size_t n_groups, size_t n_ecs) {
  return guarded(h, [&] { set_csr_impl(h, rowptr, grp, cnt, lut, lut_ld, logzi, n_groups, n_ecs); });
}

int msw_core_build_likelihood(msw_handle h, const uint64_t *ec_tptr, const uint32_t *ec_targets,
                              size_t n_ecs, const uint32_t *target_group, size_t n_targets,
                              const uint64_t *group_sizes, size_t n_groups, const uint64_t *ec_counts,
                              double q, double e, double zero_inflation, size_t min_hits,
                              size_t *n_groups_out, uint8_t *mask_out, double *logc_out) {
  return guarded(h, [&] {
    build_likelihood_impl(h, ec_tptr, ec_targets, n_ecs, target_group, n_targets, group_sizes,
                          n_groups, ec_counts, q, e, zero_inflation, min_hits, n_groups_out, mask_out,
                          logc_out, false, 0);
  });
}

int msw_core_build_likelihood_aln(msw_handle h, msw_alignment_t a, const uint32_t *target_group, size_t n_targets,
                                  const uint64_t *group_sizes, size_t n_groups, double q, double e,
                                  double zero_inflation, size_t min_hits, size_t *n_groups_out, uint8_t *mask_out,
                                  double *logc_out) {
  return guarded(h, [&] {
    if (!a) throw Fail("msw_core_build_likelihood_aln: null alignment");
    if (a->on_device && a->device == h->device) {
      // the reader's arrays are consumed where they lie (same device; the reader ran on this handle's stream or
      // has synchronised its own)
      build_likelihood_impl(h, a->d_tptr.p, a->d_targets.p, a->E, target_group, n_targets, group_sizes, n_groups,
                            a->d_counts.p, q, e, zero_inflation, min_hits, n_groups_out, mask_out, logc_out, true, a->H);
    } else {
      a->to_host(msw_alignment::kAlnTptr | msw_alignment::kAlnTargets | msw_alignment::kAlnCounts);
      build_likelihood_impl(h, a->ec_tptr.data(), a->ec_targets.data(), a->ec_counts.size(), target_group, n_targets,
                            group_sizes, n_groups, a->ec_counts.data(), q, e, zero_inflation, min_hits, n_groups_out,
                            mask_out, logc_out, false, 0);
    }
  });
}

int msw_core_layout_info(msw_handle h, msw_layout_info *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    const Resident &L = h->lik;
    if (L.flavor != 0) throw Fail("msw_core_layout_info: no CSR-of-ECs likelihood resident");
    msw_layout_info li = {};
    li.record_bytes = L.enc == kEncValue ? 12 : (L.wide() ? 8 : 4);
    li.index_records = L.hybrid() ? 1 : 0;
    li.groups_in_lds = L.glds ? 1 : 0;
    li.table_in_lds = L.tlds ? 1 : 0;
    li.passB_mode = L.gmodeB;
    li.slot_entries = L.n_area;
    li.slot_entries_in_lds = L.n_tab_lds;
    li.n_slices = L.nslices;
    li.n_long_ecs = L.n_long;
    li.bank_scheduled = L.packed_scheduled ? 1 : 0;
    li.passB_reg_cells = L.passB_rc8 ? 8 : kRegCells;
    li.rows_over_8 = L.rows_over8;
    {  // (the instantiation launch_passB_t picks: sweep_launch.hpp)
      const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
      const int rc = L.enc == kEncNarrow && L.passB_rc8 && !ml ? 8 : kRegCells;
      li.passB_waves = pass_threads_B_of(L.enc, L.gmodeB, L.tlds, rc) / kWave;
    }
    std::vector<uint32_t> off((size_t)L.nslices + 1);
    MSW_HIP(hipMemcpy(off.data(), L.slice_off.p, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    li.rows = off[L.nslices];
    for (int c = 0; c < kSliceClasses; ++c) li.slices_by_lanes[c] = L.cls.s0[c + 1] - L.cls.s0[c];
    for (uint32_t s2 = 0; s2 < L.nslices; ++s2) li.max_rows = std::max(li.max_rows, off[s2 + 1] - off[s2]);
    if (L.hybrid()) {
      std::vector<uint8_t> hot(std::max<uint32_t>(L.nslices, 1));
      MSW_HIP(hipMemcpy(hot.data(), L.slice_hot.p, hot.size(), hipMemcpyDeviceToHost));
      for (uint32_t s2 = 0; s2 < L.nslices; ++s2) li.rows_from_memory += (off[s2 + 1] - off[s2]) - hot[s2];
    } else if (!L.tlds && L.enc != kEncValue) {
      li.rows_from_memory = li.rows;
    }
    *out = li;
  });
}

int msw_core_layout_hash(msw_handle h, uint64_t *hash_out) {
  return guarded(h, [&] {
    if (!hash_out) throw Fail("null out");
    *hash_out = layout_hash(h->lik);
  });
}

int msw_core_get_dense_logl(msw_handle h, double *L_out, size_t ld) {
  return guarded(h, [&] { materialise_impl(h, L_out, ld, /*gamma=*/false, 0, h->lik.E); });
}

int msw_core_gamma(msw_handle h, double *gamma_out, size_t ld) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_gamma: no solve has run on this handle");
    materialise_impl(h, gamma_out, ld, /*gamma=*/true, 0, h->lik.E);
  });
}

int msw_core_gamma_block(msw_handle h, size_t ec_begin, size_t ec_end, double *gamma_out, size_t ld) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_gamma_block: no solve has run on this handle");
    materialise_impl(h, gamma_out, ld, /*gamma=*/true, ec_begin, ec_end);
  });
}

int msw_core_bin_reads(msw_handle h, const uint64_t *ec_rptr, const uint32_t *ec_reads, size_t n_ecs,
                       const uint32_t *targets, const double *thresholds, size_t n_targets, uint64_t *bin_ptr,
                       uint32_t *reads_out, double *log_thr_out) {
  return guarded(h, [&] {
    bin_reads_impl(h, ec_rptr, ec_reads, n_ecs, false, targets, thresholds, n_targets, bin_ptr, reads_out, log_thr_out);
  });
}

int msw_core_bin_reads_aln(msw_handle h, msw_alignment_t a, const uint32_t *targets, const double *thresholds,
                           size_t n_targets, uint64_t *bin_ptr, uint32_t *reads_out, double *log_thr_out) {
  return guarded(h, [&] {
    if (!a) throw Fail("msw_core_bin_reads_aln: null alignment");
    if (a->on_device && a->device == h->device) {
      // the reader's classes are read where they lie
      bin_reads_impl(h, a->d_rptr.p, a->d_reads.p, a->E, true, targets, thresholds, n_targets, bin_ptr, reads_out,
                     log_thr_out);
    } else {
      a->to_host(msw_alignment::kAlnRptr | msw_alignment::kAlnReads);
      bin_reads_impl(h, a->ec_rptr.data(), a->ec_reads.data(), a->ec_rptr.empty() ? 0 : a->ec_rptr.size() - 1, false,
                     targets, thresholds, n_targets, bin_ptr, reads_out, log_thr_out);
    }
  });
}

int msw_core_assign_reads(msw_handle h, const uint64_t *ec_rptr, const uint32_t *ec_reads, size_t n_ecs, const double *thresholds,
                          const uint32_t *targets, size_t n_targets, unsigned flags, uint64_t *bin_ptr, uint32_t *reads_out,
                          uint32_t *n_assigned_out, uint64_t class_reads_out[3]) {
  return guarded(h, [&] {
    assign_reads_impl(h, ec_rptr, ec_reads, n_ecs, false, thresholds, targets, n_targets, flags, bin_ptr, reads_out,
                      n_assigned_out, class_reads_out);
  });
}

int msw_core_assign_reads_aln(msw_handle h, msw_alignment_t a, const double *thresholds, const uint32_t *targets, size_t n_targets,
                              unsigned flags, uint64_t *bin_ptr, uint32_t *reads_out, uint32_t *n_assigned_out,
                              uint64_t class_reads_out[3]) {
  return guarded(h, [&] {
    assign_reads_aln_impl(h, a, thresholds, targets, n_targets, flags, bin_ptr, reads_out, n_assigned_out, class_reads_out);
  });
}

int msw_core_assign_table_rows(msw_handle h, size_t *n_rows_out) {
  return guarded(h, [&] {
    if (!n_rows_out) throw Fail("msw_core_assign_table_rows: null n_rows_out");
    assign_table_check(h, "msw_core_assign_table_rows", 0, 0);
    *n_rows_out = h->assign.n_rows;
  });
}

int msw_core_assign_table_block(msw_handle h, size_t row_begin, size_t row_end, const char **text_out, size_t *len_out) {
  return guarded(h, [&] { assign_table_plain(h, row_begin, row_end, text_out, len_out); });
}

int msw_core_assign_table_block_gzip(msw_handle h, size_t row_begin, size_t row_end, const char **out, size_t *len_out,
                                     size_t *text_len_out) {
  return guarded(h, [&] { assign_table_gzip(h, row_begin, row_end, out, len_out, text_len_out); });
}

int msw_core_set_pack_schedule(msw_handle h, int enabled) {
  return guarded(h, [&] { h->pack_schedule = enabled != 0; });
}

}  // extern "C"
