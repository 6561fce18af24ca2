// pqg_convert.hip — K10: logical-type conversion of decoded dense values (pqg_convert).
//
//   k_conv_dec<OD>    DECIMAL_BE / DECIMAL_INT of w bytes to OD little-endian dwords, sign-extended.
//                     One wave per segment of 4096 values, in tiles of at most 8 KiB of input: the
//                     tile's bytes come in as aligned 16-byte granules (the input is aligned to
//                     nothing: a dictionary read in place) into an LDS stage laid out as the input;
//                     lane L then builds value L of every group of 64 from the stage (two aligned
//                     dwords funnelled, byte-reversed by v_perm_b32, sign-filled) and stores whole
//                     aligned 16-byte granules: a KiB of contiguous output per store instruction
//                     at 16 bytes (non-temporal), two KiB by two write-back stores at 32.
//   k_conv_int96      INT96 (nanos u64, julian day i32) to int64 in a unit: the same stage; a lane
//                     takes two neighbouring values, so its store is one aligned granule.
//   k_conv_bad        BYTE_ARRAY decimals: the values whose length is 0 or above the output width
//                     or whose offsets do not lie in the chars (the count pass)
//   k_conv_bytes<OD>  BYTE_ARRAY decimals, one value per lane, read bytewise
// What a lane loads, computes and stores is pqg_convert.h (run on the host by
// tools/convert_model.cpp).  All stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "pqgpu.h"
#include "pqg_common.h"
#include "pqg_convert.h"
#include "pqg_device.h"
#include "pqg_kernels.h"

namespace pqg {

using namespace conv;

namespace {

struct GlobalIn {
  __device__ __forceinline__ Q4 ld16(uintptr_t a) const {
    const uint4 v = ldg16(a);
    return Q4{v.x, v.y, v.z, v.w};
  }
  __device__ __forceinline__ uint32_t u8(uintptr_t a) const { return *(const PQG_G uint8_t*)a; }
};

struct LdsStage {
  PQG_L uint8_t* p;
  __device__ __forceinline__ void put16(int o, const Q4& q) const { sts16(p + o, make_uint4(q.x, q.y, q.z, q.w)); }
  __device__ __forceinline__ uint32_t u32(uint32_t o) const { return *(const PQG_L uint32_t*)(p + o); }
  __device__ __forceinline__ uint32_t u8(uint32_t o) const { return p[o]; }
};

struct GlobalSink {
  __device__ __forceinline__ void st16(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    stg16o(a, make_uint4(x, y, z, w));
  }
  __device__ __forceinline__ void st16wb(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    stg16(a, make_uint4(x, y, z, w));
  }
  __device__ __forceinline__ void st8(uintptr_t a, uint32_t lo, uint32_t hi) const { stg8(a, lo, hi); }
};

// this wave's segment [s0, s1) of n values, or false
__device__ __forceinline__ bool wave_segment(int64_t n, int64_t nseg, int64_t* s0, int64_t* s1) {
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return false;
  *s0 = seg * kSeg;
  *s1 = *s0 + kSeg < n ? *s0 + kSeg : n;
  return true;
}

}  // namespace

template <int OD>
__global__ void __launch_bounds__(256) k_conv_dec(const uint8_t* in, int64_t n, int64_t nseg, int w, int be, uint8_t* out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[4][kStageBytes];
  int64_t s0, s1;
  if (!wave_segment(n, nseg, &s0, &s1)) return;
  const int lane = lane_id();
  const LdsStage st{lds_ptr(&stage[threadIdx.x >> 6][0])};
  const int T = tile_values(be ? K_DECIMAL_BE : K_DECIMAL_INT, w);
  for (int64_t t0 = s0; t0 < s1; t0 += T) {
    const int64_t t1 = t0 + T < s1 ? t0 + T : s1;
    const Tile t = tile_of((uintptr_t)in, w, t0, t1);
    stage_tile(GlobalIn{}, st, t, lane);
    __builtin_amdgcn_wave_barrier();
    const int nv = (int)(t1 - t0);
    const uintptr_t ob = (uintptr_t)out + (uintptr_t)t0 * (4 * OD);
    for (int v = lane; v < nv; v += 64) decimal_store<OD>(st, GlobalSink{}, t, w, be != 0, v, ob + (uintptr_t)v * (4 * OD));
    // the next tile's LDS writes come after this tile's reads (one wave: DS operations in order)
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void __launch_bounds__(256) k_conv_int96(const uint8_t* in, int64_t n, int64_t nseg, int unit, uint8_t* out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[4][kStageBytes];
  int64_t s0, s1;
  if (!wave_segment(n, nseg, &s0, &s1)) return;
  const int lane = lane_id();
  const LdsStage st{lds_ptr(&stage[threadIdx.x >> 6][0])};
  const int T = tile_values(K_INT96_TIME, 12);
  for (int64_t t0 = s0; t0 < s1; t0 += T) {
    const int64_t t1 = t0 + T < s1 ? t0 + T : s1;
    const Tile t = tile_of((uintptr_t)in, 12, t0, t1);
    stage_tile(GlobalIn{}, st, t, lane);
    __builtin_amdgcn_wave_barrier();
    const int nv = (int)(t1 - t0);
    const uintptr_t ob = (uintptr_t)out + (uintptr_t)t0 * 8;
    for (int p = lane; 2 * p < nv; p += 64) int96_store(st, GlobalSink{}, t, unit, p, nv, ob + 16 * (uintptr_t)p);
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void __launch_bounds__(256) k_conv_bad(const int64_t* offsets_, int64_t n, int64_t nseg, int64_t values_bytes,
                                                  int ow, unsigned long long* bad) {
  int64_t s0, s1;
  if (!wave_segment(n, nseg, &s0, &s1)) return;
  const PQG_G int64_t* offsets = gconst(offsets_);
  const int lane = lane_id();
  int64_t nb = 0;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    nb += __popcll(__ballot(i < s1 && bytes_len(offsets[i], offsets[i + 1], values_bytes, ow) < 0));
  }
  if (lane == 0 && nb) atomicAdd(bad, (unsigned long long)nb);
}

template <int OD>
__global__ void __launch_bounds__(256) k_conv_bytes(const uint8_t* values, const int64_t* offsets_, int64_t n, int64_t nseg,
                                                    int64_t values_bytes, uint8_t* out) {
  int64_t s0, s1;
  if (!wave_segment(n, nseg, &s0, &s1)) return;
  const PQG_G int64_t* offsets = gconst(offsets_);
  const GlobalSink sink{};
  for (int64_t i = s0 + lane_id(); i < s1; i += 64) {
    const int64_t o0 = offsets[i], len = bytes_len(o0, offsets[i + 1], values_bytes, 4 * OD);
    if (len < 0) continue;  // the count pass found none: nothing is read or written for one
    uint32_t o[OD];
    bytes_value<OD>(GlobalIn{}, (uintptr_t)values + (uintptr_t)o0, (int)len, o);
    const uintptr_t at = (uintptr_t)out + (uintptr_t)i * (4 * OD);
    sink.st16(at, o[0], o[1], o[2], o[3]);
    if constexpr (OD == 8) sink.st16(at + 16, o[4], o[5], o[6], o[7]);
  }
}

// ---- host launchers (called from pqg_convert in pqg_ops.hip) --------------------------------------

static unsigned conv_blocks(int64_t n, int64_t* nseg) {
  *nseg = (n + kSeg - 1) / kSeg;
  return (unsigned)((*nseg + 3) / 4);
}

// BYTE_ARRAY decimals: tot[0] = the bad values (zeroed here)
int convert_count_launch(hipStream_t s, const pqg_convert_args* a, int64_t* tot) {
  int64_t nseg;
  const unsigned blocks = conv_blocks(a->num_values, &nseg);
  if (hipMemsetAsync(tot, 0, sizeof(int64_t), s) != hipSuccess) return PQG_ERR_HIP;
  hipLaunchKernelGGL(k_conv_bad, dim3(blocks), dim3(256), 0, s, a->offsets, a->num_values, nseg, a->values_bytes,
                     a->out_width, (unsigned long long*)tot);
  return hipGetLastError() == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

// the write pass of checked arguments (num_values > 0)
int convert_launch(hipStream_t s, const pqg_convert_args* a) {
  int64_t nseg;
  const unsigned blocks = conv_blocks(a->num_values, &nseg);
  const int64_t n = a->num_values;
  const bool wide = a->out_width == 32;
  if (a->kind == PQG_CONV_INT96_TIME) {
    hipLaunchKernelGGL(k_conv_int96, dim3(blocks), dim3(256), 0, s, a->values, n, nseg, a->unit, a->out);
  } else if (a->offsets) {
    if (wide)
      hipLaunchKernelGGL(k_conv_bytes<8>, dim3(blocks), dim3(256), 0, s, a->values, a->offsets, n, nseg, a->values_bytes, a->out);
    else
      hipLaunchKernelGGL(k_conv_bytes<4>, dim3(blocks), dim3(256), 0, s, a->values, a->offsets, n, nseg, a->values_bytes, a->out);
  } else {
    const int be = a->kind == PQG_CONV_DECIMAL_BE;
    if (wide)
      hipLaunchKernelGGL(k_conv_dec<8>, dim3(blocks), dim3(256), 0, s, a->values, n, nseg, a->in_width, be, a->out);
    else
      hipLaunchKernelGGL(k_conv_dec<4>, dim3(blocks), dim3(256), 0, s, a->values, n, nseg, a->in_width, be, a->out);
  }
  return hipGetLastError() == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

}  // namespace pqg
