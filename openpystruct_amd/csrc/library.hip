// Library-wide host state: the last error (ops_amd_last_error), the ABI version, and the library options -- ops_amd_set_option is the one place
// a caller (tests, A/B scripts) steers the dispatch; no environment variable is read.  library.hpp's launch_status and
// launch_refused, the one place that returns OPS_AMD_ERR_LAUNCH, store their message here.  No kernels.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <string_view>

#include "../../include/openpystruct_amd.h"
#include "library.hpp"

static thread_local char g_last_error[256] = {0};

static std::atomic<long> g_frame_latency_batch{-1};
static std::atomic<long> g_frame_coop{1};
static std::atomic<long> g_frame_pack{1};
static std::atomic<int> g_deterministic{0};

namespace opsamd {

void set_last_error(const char* msg) {
  int k = 0;
  for (; msg && msg[k] && k < 255; ++k) g_last_error[k] = msg[k];
  g_last_error[k] = 0;
}

int current_device(int* devid) {
  const hipError_t e = hipGetDevice(devid);
  if (e != hipSuccess) {
    char why[256];
    snprintf(why, sizeof(why), "hipGetDevice failed: %s", hipGetErrorString(e));
    return launch_refused(why);
  }
  return *devid >= 0 && *devid < 64 ? OPS_AMD_OK : launch_refused("device index outside 0..63");
}

int deterministic_mode() { return g_deterministic.load(std::memory_order_relaxed); }
long frame_latency_batch_option() { return g_frame_latency_batch.load(); }
long frame_coop_option() { return g_frame_coop.load(); }
long frame_pack_option() { return g_frame_pack.load(); }

}  // namespace opsamd

extern "C" int ops_amd_abi_version(void) { return OPS_AMD_ABI_VERSION; }
extern "C" const char* ops_amd_last_error(void) { return g_last_error; }

extern "C" int ops_amd_set_option(const char* name, long value) {
  if (!name) return OPS_AMD_ERR_INVALID_ARG;
  const std::string_view n(name);
  if (n == "frame_latency_batch") { g_frame_latency_batch.store(value < 0 ? -1 : value); return OPS_AMD_OK; }
  if (n == "frame_pack") { g_frame_pack.store(value != 0); return OPS_AMD_OK; }
  if (n == "frame_coop") { if (value < 0 || value > 2) return OPS_AMD_ERR_INVALID_ARG; g_frame_coop.store(value); return OPS_AMD_OK; }
  if (n == "deterministic") { g_deterministic.store(value != 0); return OPS_AMD_OK; }
  return OPS_AMD_ERR_INVALID_ARG;
}
extern "C" long ops_amd_get_option(const char* name) {
  if (!name) return -2;
  const std::string_view n(name);
  if (n == "frame_latency_batch") return g_frame_latency_batch.load();
  if (n == "frame_pack") return g_frame_pack.load();
  if (n == "frame_coop") return g_frame_coop.load();
  if (n == "deterministic") return g_deterministic.load();
  return -2;
}
