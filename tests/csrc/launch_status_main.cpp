// The launch epilogue of csrc/library.hip on the host, without a GPU (tests/test_launch_status.py builds this file together with
// library.hip and runs it).  Only the overload that is handed an error is called: the one without arguments asks the runtime,
// whose answer without a device is its own.  Prints the first statement that does not hold and exits 1; "ok" and 0 otherwise.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "../../include/openpystruct_amd.h"
#include "../../openpystruct_amd/csrc/library.hpp"

#define CHECK(cond)                                                                                            \
  do {                                                                                                         \
    if (!(cond)) {                                                                                             \
      std::printf("line %d: %s does not hold (last error: \"%s\")\n", __LINE__, #cond, ops_amd_last_error()); \
      return 1;                                                                                                \
    }                                                                                                          \
  } while (0)

using namespace opsamd;

static bool last_is(const char* text) { return std::strcmp(ops_amd_last_error(), text) == 0; }

int main() {
  // success: OPS_AMD_OK, the stored message as it was -- empty
  CHECK(last_is(""));
  CHECK(launch_status(hipSuccess) == OPS_AMD_OK);
  CHECK(last_is(""));

  // a failure: the code, and HIP's text for it
  const std::string config = hipGetErrorString(hipErrorInvalidConfiguration), value = hipGetErrorString(hipErrorInvalidValue);
  CHECK(!config.empty() && !value.empty() && config != value);
  CHECK(launch_status(hipErrorInvalidConfiguration) == OPS_AMD_ERR_LAUNCH);
  CHECK(last_is(config.c_str()));

  // success again: the stored message as it was -- set
  CHECK(launch_status(hipSuccess) == OPS_AMD_OK);
  CHECK(last_is(config.c_str()));

  // the next failure replaces the text
  CHECK(launch_status(hipErrorInvalidValue) == OPS_AMD_ERR_LAUNCH);
  CHECK(last_is(value.c_str()));

  // a refusal: the code and the caller's words, the first 255 characters of them
  CHECK(launch_refused("x") == OPS_AMD_ERR_LAUNCH);
  CHECK(last_is("x"));
  const std::string text(400, 'q');
  CHECK(launch_refused(text.c_str()) == OPS_AMD_ERR_LAUNCH);
  CHECK(last_is(std::string(255, 'q').c_str()));

  // the store is per thread: another thread starts empty, and what it stores stays its own
  std::string seen = "unset", seen_after;
  std::thread([&] {
    seen = ops_amd_last_error();
    launch_refused("other thread");
    seen_after = ops_amd_last_error();
  }).join();
  CHECK(seen.empty());
  CHECK(seen_after == "other thread");
  CHECK(last_is(std::string(255, 'q').c_str()));

  std::printf("ok\n");
  return 0;
}
