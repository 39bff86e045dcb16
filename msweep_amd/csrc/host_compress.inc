// host_compress.inc -- msw_core_set_dense_logl's fast path (included by build.hip): the
// matrix the reference hands to rcg_optl (src/mSWEEP.cpp:194-202, built by
// include/Likelihood.hpp:176-185) holds log(zi) in every cell whose EC does not hit the group and
// one of a few lookup-table values elsewhere.  When the staged matrix has that shape it is
// re-expressed -- on the device, exactly -- as CSR-of-ECs + value table and solved by the SELL
// sweeps (tens of bytes per listed cell and iteration instead of 16 bytes per cell of G x E).
namespace {

constexpr uint32_t kCompressMaxValues = 1u << 24;  // distinct listed values (each costs two exp per iteration)
constexpr uint32_t kCompressShared = 1u << 16;     // up to here equal values share a slot (tables can sit in LDS)
constexpr size_t kCompressSample = 4096;

// stage: the matrix on the device, [G][E] contiguous; Lm: the same matrix on the host, or null (the background sample
// is then read from the stage).  True = h now holds the CSR flavour.
// force: the matrix has more groups than the dense sweeps take (dense_kernels.hpp: 8192) -- it is re-expressed
// whatever its shape (most frequent sampled value as the background, every other cell listed with a slot of its
// own), up to 2^28 listed cells.
bool compress_dense(msw_core *h, const double *Lm, size_t ld, const double *stage, size_t G, size_t E, bool force) {
  Resident &L = h->lik;
  const char *sw = getenv("MSWEEP_DENSE_COMPRESS");  // developer switch: 0 = always the dense sweeps
  if (sw && atoi(sw) == 0 && !force) return false;
  if (G > 0x7fffffffull) return false;
  // background candidate: the most frequent value of a host-side sample; must hold half of it
  uint64_t bg = 0;
  {
    std::unordered_map<uint64_t, uint32_t> seen;
    const size_t cells = G * E, n = std::min(cells, kCompressSample);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    // the sampled cells, as indices into the [G][E] stage, and their bits: from the host matrix, or -- Lm null, a matrix
    // that never was on the host (host_likelihood_file.inc) -- the same cells fetched from the stage (<= 32 KB)
    std::vector<uint64_t> at(n), val(n);
    for (size_t i = 0; i < n; ++i) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      at[i] = cells <= kCompressSample ? i : (size_t)((x >> 11) % cells);
    }
    if (Lm) {
      for (size_t i = 0; i < n; ++i) std::memcpy(&val[i], &Lm[(at[i] / E) * ld + at[i] % E], sizeof(uint64_t));
    } else {
      DevBuf<uint64_t> d_at;
      DevBuf<double> d_val;
      d_at.upload(at.data(), n, h->stream);
      d_val.alloc(n);
      lik_gather_launch(h->stream, stage, d_at.p, (uint32_t)n, d_val.p);  // (k_lik_gather: input.hip)
      MSW_HIP(hipGetLastError());
      MSW_HIP(hipMemcpyAsync(val.data(), d_val.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
      MSW_HIP(hipStreamSynchronize(h->stream));
    }
    uint32_t best = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t v = val[i];
      const uint32_t k = ++seen[v];
      if (k > best) {
        best = k;
        bg = v;
      }
    }
    double b;
    std::memcpy(&b, &bg, sizeof b);
    if (!std::isfinite(b)) {
      if (!force) return false;
      // (-inf cells cannot be the background of the sweeps: any finite value will do, its cells are just listed)
      const double z = -1.0;
      std::memcpy(&bg, &z, sizeof z);
    } else if (2 * (size_t)best < n && !force) {
      return false;
    }
  }
  hipStream_t st = h->stream;
  const uint64_t *bits = reinterpret_cast<const uint64_t *>(stage);
  const unsigned nbe = (unsigned)std::min<size_t>((E + 256) / 256, (size_t)h->n_cu * 16);
  DevBuf<uint32_t> d_rowptr, tot;
  DevBuf<uint64_t> gt;
  d_rowptr.alloc(E + 1);
  hipLaunchKernelGGL(k_dense_count, dim3(nbe), dim3(256), 0, st, bits, (uint32_t)G, (uint32_t)E, bg, d_rowptr.p);
  MSW_HIP(hipGetLastError());
  const uint64_t nnz = device_scan_u32(h, d_rowptr.p, E + 1, tot, gt);
  if (force && nnz >= (1ull << 28))
    throw Fail("msw_core_set_dense_logl: more than 8192 groups and 2^28 or more cells that differ from the most "
               "frequent value: use the CSR-of-ECs form");
  if (!force && (nnz >= 0xffffffffull || nnz * 4 > (uint64_t)G * E)) return false;
  DevBuf<uint32_t> d_grp, d_pos, d_pos2, d_idx, d_head;
  DevBuf<uint64_t> d_val, d_val2, d_lut;
  d_grp.alloc(nnz);
  d_val.alloc(nnz);
  d_pos.alloc(nnz);
  uint64_t n_values = 0;
  bool value_records = false;
  d_idx.alloc(nnz);
  if (nnz) {
    hipLaunchKernelGGL(k_dense_extract, dim3(nbe), dim3(256), 0, st, bits, (uint32_t)G, (uint32_t)E, bg, d_rowptr.p,
                       d_grp.p, d_val.p, d_pos.p);
    // distinct values: sort (value, cell), flag the first cell of every value, rank by prefix sum
    d_val2.alloc(nnz);
    d_pos2.alloc(nnz);
    size_t tmp_bytes = 0;
    MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, d_val.p, d_val2.p, d_pos.p, d_pos2.p, (size_t)nnz, 64u, st));
    DevBuf<unsigned char> tmp;
    tmp.alloc(tmp_bytes);
    MSW_HIP(prim_sort_pairs(tmp.p, tmp_bytes, d_val.p, d_val2.p, d_pos.p, d_pos2.p, (size_t)nnz, 64u, st));
    d_head.alloc(nnz);
    const unsigned nbn = (unsigned)std::min<uint64_t>((nnz + 255) / 256, (uint64_t)h->n_cu * 32);
    hipLaunchKernelGGL(k_value_heads, dim3(nbn), dim3(256), 0, st, d_val2.p, nnz, d_head.p);
    MSW_HIP(hipGetLastError());
    n_values = device_scan_u32(h, d_head.p, nnz, tot, gt) + 1;
    if (n_values > kCompressMaxValues && !force) return false;
    if (n_values > kCompressShared) {
      // (nearly) every listed cell has its own value: the tables cannot live in LDS anyway, so give
      // cell k slot k -- an EC's table entries are then neighbours in memory, like its records
      n_values = nnz;
      d_lut.alloc(nnz);
      MSW_HIP(hipMemcpyAsync(d_lut.p, d_val.p, nnz * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      MSW_HIP(hipMemcpyAsync(d_idx.p, d_pos.p, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      // ... or better, no table at all: VALUE RECORDS (sell.hpp) carry the cell's log-likelihood and the sweeps
      // form its exponential themselves -- 12 bytes per cell and sweep instead of 8 + 16 gathered + 40 rebuilt
      const char *vr = getenv("MSWEEP_VALUE_RECORDS");  // developer switch: 0 = the slot per cell
      value_records = !(vr && atoi(vr) == 0);
    } else {
      d_lut.alloc(n_values);
      hipLaunchKernelGGL(k_value_ranks, dim3(nbn), dim3(256), 0, st, d_val2.p, d_pos2.p, d_head.p, nnz, d_idx.p, d_lut.p);
      MSW_HIP(hipGetLastError());
    }
  }
  L.G = (uint32_t)G;
  L.E = (uint32_t)E;
  L.nnz = nnz;
  std::memcpy(&L.logzi, &bg, sizeof bg);
  if (value_records) {
    L.n_lut = 1;
    L.lut.alloc(1);
    MSW_HIP(hipMemcpyAsync(L.lut.p, &L.logzi, sizeof(double), hipMemcpyHostToDevice, st));
    sell_from_device(h, d_rowptr.p, d_grp.p, d_idx.p, reinterpret_cast<const double *>(d_lut.p));  // synchronises
    return true;
  }
  L.n_lut = (uint32_t)std::max<uint64_t>(n_values, 1);
  L.lut.alloc(L.n_lut);
  if (n_values)
    MSW_HIP(hipMemcpyAsync(L.lut.p, d_lut.p, n_values * sizeof(double), hipMemcpyDeviceToDevice, st));
  else
    MSW_HIP(hipMemcpyAsync(L.lut.p, &L.logzi, sizeof(double), hipMemcpyHostToDevice, st));
  sell_from_device(h, d_rowptr.p, d_grp.p, d_idx.p);  // synchronises
  return true;
}

}  // namespace
