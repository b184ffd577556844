// The scaffold of the streaming kernels around the batched frame solve (device only): csrc/frame_vjp.hip, frame_sizing_grad.hip
// and frame_loads.hip.  They are one thread per output row -- (frame, node) or (frame, element), the
// frame slowest, so a wave's stores are one contiguous run and its loads are runs of neighbouring rows -- over a grid-stride
// loop; no LDS, no atomics: every output is one thread's sum in a fixed order.  Stated here once: the block size and the grid
// cap, the row division, the topology pointers every params struct opens with, the row loop and the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/openpystruct_amd.h"
#include "library.hpp"

namespace opsamd {

constexpr int FRAME_STREAM_BLOCK = 256;
constexpr long FRAME_STREAM_MAX_GRID = 2048;     // memory-bound: a few workgroups per CU, the rest of the rows by grid stride

// what every streaming kernel's params struct opens with (a kernel that does not read a field is not given it)
struct FrameStreamTopo {
  int B, Nn, Ne;
  const double* elem_geo;          // [Ne,3]  L, cos, sin
  const double* elem_EA;           // [Ne]
  const double* elem_E;            // [Ne]
  const int32_t* conn;             // [Ne,2]
  const int32_t* node_elem_ptr;    // [Nn+1]
  const int32_t* node_elem_idx;    // [2 Ne]  2 * element + end
};

// frame of row i of `total` rows, `per` rows to a frame: a 32-bit division wherever the row count allows (the 64-bit one is a
// long instruction sequence on this target); `small` is uniform over the launch
__device__ __forceinline__ long row_frame(long i, int per, bool small) {
  return small ? (long)((unsigned)i / (unsigned)per) : i / per;
}

// body(i, b, j) for every row i of B frames of `per` rows this thread serves: row j of frame b
template <class Body>
__device__ __forceinline__ void frame_stream_rows(int B, int per, Body body) {
  const long total = (long)B * per, stride = (long)gridDim.x * FRAME_STREAM_BLOCK;
  for (long i = (long)blockIdx.x * FRAME_STREAM_BLOCK + threadIdx.x; i < total; i += stride) {
    const long b = row_frame(i, per, total <= 0x7fffffffL);
    body(i, b, (int)(i - b * per));
  }
}

// one thread per row up to the grid cap; a launch error is reported through ops_amd_last_error
template <class Params>
int frame_stream_launch(void (*kernel)(const Params), const Params& p, long rows, void* stream) {
  const long need = (rows + FRAME_STREAM_BLOCK - 1) / FRAME_STREAM_BLOCK;
  const unsigned grid = (unsigned)(need < FRAME_STREAM_MAX_GRID ? need : FRAME_STREAM_MAX_GRID);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(FRAME_STREAM_BLOCK), 0, (hipStream_t)stream, p);
  return launch_status();
}

}  // namespace opsamd
