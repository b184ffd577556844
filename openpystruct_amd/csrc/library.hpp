// Library-wide host state (csrc/library.hip): the last error, the options of ops_amd_set_option, and the once-per-device kernel setup.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/openpystruct_amd.h"

namespace opsamd {

void set_last_error(const char* msg);   // what ops_amd_last_error() reports (per thread)

// The one epilogue of an entry that launches: every OPS_AMD_ERR_LAUNCH of the library is returned through one of these, so the code
// never comes without its message.  hipSuccess: OPS_AMD_OK and the stored message untouched; else HIP's text for `e` is stored.
// Inline over set_last_error: a file built alone (mlp_block.hip under MB_EXP) needs that one symbol and no more, as before.
inline int launch_refused(const char* why) { set_last_error(why); return OPS_AMD_ERR_LAUNCH; }      // a launch the entry would not make
inline int launch_status(hipError_t e) { return e != hipSuccess ? launch_refused(hipGetErrorString(e)) : OPS_AMD_OK; }
inline int launch_status() { return launch_status(hipGetLastError()); }
int current_device(int* devid);         // OPS_AMD_OK and the current device's index, or the refusal: hipGetDevice failed, an index outside 0 .. 63

// library options (ops_amd_set_option / ops_amd_get_option)
int deterministic_mode();               // "deterministic": fixed-order reductions in the Transformer-Diffusion step's gradient launches
long frame_latency_batch_option();      // "frame_latency_batch": -1 = the dispatch model of frame_solve.hip; n >= 0: the tuned kernels above n frames
long frame_coop_option();               // "frame_coop": 0 = never four waves per frame; 1 = where measured faster; 2 = for every small batch
long frame_pack_option();               // "frame_pack": 0 = one wave per frame for every half bandwidth

// Raises kernel `Fn`'s dynamic-LDS limit to `bytes` on device `devid` (0 .. 63), once per device: the limit is a per-DEVICE function attribute
// and a process may drive several GPUs (ops.set_device / FrameTopology(device=...)).  Two threads racing here both set the same value.
template <auto Fn>
static hipError_t set_lds_limit_once(int devid, int bytes) {
  static std::atomic<unsigned long long> done{0};
  const unsigned long long bit = 1ull << devid;
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)Fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

}  // namespace opsamd
