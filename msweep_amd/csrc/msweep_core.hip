// msweep_core.hip -- the C ABI of libmsweep_core.so (include/msweep_core.h): the handle's creation and destruction and
// the version string.  The entries of every family sit in the translation unit of its host code -- solve.hip, build.hip,
// input.hip, output.hip -- and the sweeps in sweep_<encoding>.hip and sweep_dense.hip (host_api.hpp: what the units call in one another).
//
// No CPU fallback exists in this library: every numeric step of the hot path (likelihood
// expansion, RCG / EM sweeps, column reductions, ELBO, bootstrap resampling) is a HIP
// kernel; the host only validates shapes, lays out buffers and enqueues launches.
#include "host_api.hpp"

thread_local std::string msw::host::g_create_error;

void msw::host::grant_dynamic_lds(const void *kernel, size_t bytes) {
  static msw::LdsGrants grants;  // (the one process-wide table of the library besides the code objects themselves)
  int device = 0;
  MSW_HIP(hipGetDevice(&device));
  grants.raise(device, kernel, bytes, [&](size_t b) {
    MSW_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b));
  });
}

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

#ifndef MSW_SRC_HASH
#define MSW_SRC_HASH "unhashed"
#endif
// "... src <hash>": sha256 prefix of the sources this library was compiled from (__graft_entry__.source_hash)
const char *msw_core_version(void) { return "msweep_core 0.2 gfx950 (HIP, wave64) src " MSW_SRC_HASH; }

const char *msw_last_error(msw_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msw_core_create(int device, msw_handle *out) {
  if (!out) return 1;
  *out = nullptr;
  try {
    int n = 0;
    MSW_HIP(hipGetDeviceCount(&n));
    if (n <= 0) throw Fail("no HIP device visible: libmsweep_core has no CPU fallback");
    if (device < 0 || device >= n) throw Fail("device index out of range");
    MSW_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MSW_HIP(hipGetDeviceProperties(&prop, device));
    std::unique_ptr<msw_core> h(new msw_core);
    h->device = device;
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    MSW_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->solver.stream = h->stream;
    h->solver.n_cu = h->n_cu;
    // code object load: here, once per process -- every unit's, each loaded by the first launch out of it
    for (auto warm : {warm_solve, warm_build, warm_input, warm_output, warm_prim, warm_sweep_narrow, warm_sweep_wide,
                      warm_sweep_index, warm_sweep_dense})
      warm(h->stream);
    MSW_HIP(hipGetLastError());
    MSW_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    return 1;
  }
}

void msw_core_destroy(msw_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

}  // extern "C"
