// Host side shared by the bfmmm_post_* entry points (kernels_post.hip, kernels_bands.hip, kernels_loo.hip, kernels_diag.hip):
// the functions they call in each other's files, device selection, an owning list of device buffers and the event pair that
// times a call's kernels.  capi_chain.hpp has its own CallBufs, which reports hipError_t and owns events as well.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

int bfmmm_io_fail(const std::string& m);      // entry_points.cpp: sets bfmmm_entry_last_error, returns 1
void bfmmm_post_set_kernel_ms(float ms);      // kernels_post.hip: what bfmmm_post_last_kernel_ms returns
// kernels_loo.hip: the PSIS / WAIC pass over n rows of S values on the current device (also in launchers.hpp, for capi_loo.hip)
int post_psis_device(const double* d_ll, long long ld, int n, int S, double* const out[6]);
int post_psis_expect_device(const double* d_ll, long long ld, int n, int S, const double* d_aux, int n_aux, long long aux_stride,
                            double* const out[6], double* expect_host);

namespace {      // internal to each including file: the library exports nothing from here

// makes `device` current; otherwise reports "<who>: ..." and returns 1
int select_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return bfmmm_io_fail(std::string(who) + ": no HIP device (the MI355X library has no CPU path)");
  if (hipSetDevice(device) != hipSuccess) return bfmmm_io_fail(std::string(who) + ": cannot select the device");
  return 0;
}

// device buffers of one call, freed when it returns
struct DevBufs {
  std::vector<void*> p;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() { for (void* q : p) (void)hipFree(q); }
  // *out = a buffer of max(count, 1) elements, filled from host where host is not null; false: allocation or copy failed
  template <class Tp>
  bool put(Tp** out, const Tp* host, size_t count) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(Tp)) != hipSuccess) return false;
    p.push_back(d);
    if (host && count && hipMemcpy(d, host, count * sizeof(Tp), hipMemcpyHostToDevice) != hipSuccess) return false;
    *out = (Tp*)d;
    return true;
  }
  template <class Tp>
  bool put(Tp** out, std::nullptr_t, size_t count) { return put(out, (const Tp*)nullptr, count); }
};

// Runs enqueue() (launches on the default stream; false: it could not launch) between two events and waits for the device.
// True: everything ran, and the device time between the events went to bfmmm_post_set_kernel_ms.
template <class F>
bool timed_launch(F&& enqueue) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, 0);
  const bool launched = enqueue();
  (void)hipEventRecord(e1, 0);
  const bool ran = launched && hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
  if (ran) { float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1); bfmmm_post_set_kernel_ms(ms); }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return ran;
}

}  // namespace
