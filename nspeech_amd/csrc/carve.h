// One declaration per memory layout.  A kernel's dynamic LDS, and a launcher's work area, is a run of packed arrays;
// a layout struct carves it once - the arrays taken in order, each byte offset and the total kept - and both the kernel
// (pointers) and the launcher (bytes to ask for, bytes to clear) read that one struct:
//   struct GenLds {                                 // dynamic LDS of wn_generate_kernel
//     int R, Dc;                                    // what the carve depends on (template parameters where it can be)
//     LdsCarve c = {};
//     int xin = c.take<float>(2 * R);               // [2R]: x[t-d] | x[t]
//     int z = c.take<float>(2 * Dc);                // [2Dc]
//     int bytes = c.off;
//   };
//   kernel:    const GenLds lay{R, Dc};  float* z = carve_at<float>(smem, lay.z);
//   launcher:  hipLaunchKernelGGL(..., GenLds{p->R, p->Dc}.bytes, ...)
// No padding is ever added: the images are packed, and an array that needs an alignment gets it from the sizes in
// front of it.  Say so where it matters: static_assert(carve_aligned(lay.wl, 16)) where the layout is a constant
// expression, NS_CHECK_ARG(carve_aligned(lay.ex, 8), ...) in the launcher where it depends on run-time shapes.
#pragma once
#include <stddef.h>

template <typename O>
struct CarveT {
  O off = 0;
  // byte offset of the next array of count T; advances past it
  template <typename T>
  __host__ __device__ constexpr O take(O count) {
    const O o = off;
    off += count * (O)sizeof(T);
    return o;
  }
};
// LDS offsets are ints: a layout stays far below 2^31, and 32-bit offsets leave the kernels' address arithmetic (and so
// their register counts) as the hand-written float* chains had it; work areas in global memory count in size_t
using LdsCarve = CarveT<int>;
using WorkCarve = CarveT<size_t>;

template <typename O>
__host__ __device__ constexpr bool carve_aligned(O off, int align) { return off % align == 0; }
// the size of a region that two layouts overlay
template <typename O>
__host__ __device__ constexpr O max_of(O a, O b) { return a > b ? a : b; }

// the array at byte offset off of a carved region
template <typename T, typename O>
__host__ __device__ __forceinline__ T* carve_at(void* base, O off) { return (T*)((char*)base + off); }
