// NIfTI-1 voxels of decoded payloads to the arrays nifti.load returns (values_amd/nifti.py: load_device) -- the inverse
// of nifti_payload.hip.  One launch decodes a batch: per item, the voxels at src + vox_offset, stored in Fortran order
// (x fastest), go to dst in C order, indexed [x, y, z, ...]:
//
//   3-D items: a 64 x 64 (x, z) tile of one y per workgroup, as nifti_payload_kernel in the other direction -- the reads
//     run along x (the file's fastest axis), the tile goes through LDS, the writes run along z (the output's fastest
//     axis), both coalesced;
//   any other rank (1-D to 7-D): a gather, one output element per lane, its Fortran index from its C coordinates.
//
// Elements are byte-swapped for a big-endian file.  A scaled item (scl_slope / scl_inter) is written as
// v * slope + inter in the type numpy promotes a * slope + inter to: float32 operands for a float32 file, float64 for
// the rest (the Makefile builds with -ffp-contract=off: no fused multiply-add changes a rounding).
#include <vector>

#include "common.h"

namespace {

constexpr int ND_TILE = 64;

struct NdItemDev {
  vx_nifti_dec_item it;
  int64_t block0;    // first workgroup of the item in the launch
  int64_t nvox;
  int32_t esize;     // file element bytes
  int32_t out_es;    // output element bytes
  int32_t tiled;     // 3-D tile path
  int32_t aligned;   // src + vox_offset aligned to esize
  int32_t tx, tz;    // tiles along x and z
};

__device__ __forceinline__ uint64_t nd_load(const NdItemDev& d, int64_t f) {
  const uint8_t* p = d.it.src + d.it.vox_offset + f * d.esize;
  uint64_t v = 0;
  if (d.aligned) {
    switch (d.esize) {
      case 1: v = *p; break;
      case 2: v = *reinterpret_cast<const uint16_t*>(p); break;
      case 4: v = *reinterpret_cast<const uint32_t*>(p); break;
      default: v = *reinterpret_cast<const uint64_t*>(p); break;
    }
  } else {
    for (int k = 0; k < d.esize; ++k) v |= (uint64_t)p[k] << (8 * k);
  }
  if (d.it.big_endian && d.esize > 1) {
    v = __builtin_bswap64(v) >> (64 - 8 * d.esize);
  }
  return v;
}

__device__ __forceinline__ double nd_as_double(uint64_t v, int code) {
  switch (code) {
    case 2: return (double)(uint8_t)v;
    case 4: return (double)(int16_t)(uint16_t)v;
    case 8: return (double)(int32_t)(uint32_t)v;
    case 16: return (double)__uint_as_float((uint32_t)v);
    case 64: return __longlong_as_double((long long)v);
    case 256: return (double)(int8_t)(uint8_t)v;
    case 512: return (double)(uint16_t)v;
    case 768: return (double)(uint32_t)v;
    case 1024: return (double)(int64_t)v;
    default: return (double)v;   // 1280: uint64
  }
}

// element bits of the file type -> output element bits
__device__ __forceinline__ uint64_t nd_convert(const NdItemDev& d, uint64_t v) {
  if (d.it.out_dtype == VX_F32) {
    const float r = __uint_as_float((uint32_t)v) * (float)d.it.slope + (float)d.it.inter;
    return __float_as_uint(r);
  }
  if (d.it.out_dtype == VX_F64) {
    const double r = nd_as_double(v, d.it.code) * d.it.slope + d.it.inter;
    return (uint64_t)__double_as_longlong(r);
  }
  return v;
}

__device__ __forceinline__ void nd_store(const NdItemDev& d, int64_t i, uint64_t v) {
  uint8_t* o = reinterpret_cast<uint8_t*>(d.it.dst);
  switch (d.out_es) {
    case 1: o[i] = (uint8_t)v; break;
    case 2: reinterpret_cast<uint16_t*>(o)[i] = (uint16_t)v; break;
    case 4: reinterpret_cast<uint32_t*>(o)[i] = (uint32_t)v; break;
    default: reinterpret_cast<uint64_t*>(o)[i] = v; break;
  }
}

__global__ __launch_bounds__(256) void nifti_decode_kernel(const NdItemDev* __restrict__ items, int n_items) {
  __shared__ uint64_t tile[ND_TILE][ND_TILE + 1];
  const int tid = threadIdx.x;
  int lo = 0, hi = n_items - 1;
  const int64_t blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= blk) lo = mid;
    else hi = mid - 1;
  }
  const NdItemDev& d = items[lo];
  const int64_t k = blk - d.block0;
  if (!d.tiled) {
    const int64_t i = k * 256 + tid;
    if (i >= d.nvox) return;
    // C coordinates of output element i -> Fortran index
    int64_t r = i, f = 0, fs = 1;
    int64_t c[7];
#pragma unroll
    for (int a = 6; a >= 0; --a) {
      if (a < d.it.ndim) {
        const int64_t n = d.it.dims[a];
        c[a] = r % n;
        r /= n;
      }
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      if (a < d.it.ndim) {
        f += c[a] * fs;
        fs *= d.it.dims[a];
      }
    }
    nd_store(d, i, nd_convert(d, nd_load(d, f)));
    return;
  }
  const int X = d.it.dims[0], Y = d.it.dims[1], Z = d.it.dims[2];
  const int zt = (int)(k % d.tz);
  const int xt = (int)((k / d.tz) % d.tx);
  const int y = (int)(k / ((int64_t)d.tz * d.tx));
  const int x0 = xt * ND_TILE, z0 = zt * ND_TILE;
  {   // read along x: file element (z * Y + y) * X + x
    const int xx = tid & 63, x = x0 + xx;
    for (int zz = tid >> 6; zz < ND_TILE; zz += 4) {
      const int z = z0 + zz;
      if (x < X && z < Z) tile[xx][zz] = nd_convert(d, nd_load(d, ((int64_t)z * Y + y) * X + x));
    }
  }
  __syncthreads();
  {   // write along z: output element (x * Y + y) * Z + z
    const int zz = tid & 63, z = z0 + zz;
    for (int xx = tid >> 6; xx < ND_TILE; xx += 4) {
      const int x = x0 + xx;
      if (x < X && z < Z) nd_store(d, ((int64_t)x * Y + y) * Z + z, tile[xx][zz]);
    }
  }
}

int nd_esize(int code) {
  switch (code) {
    case 2: case 256: return 1;
    case 4: case 512: return 2;
    case 8: case 16: case 768: return 4;
    case 64: case 1024: case 1280: return 8;
    default: return 0;
  }
}

}  // namespace

extern "C" int64_t vx_nifti_decode_workspace_bytes(int n_items) {
  if (n_items < 0) return -1;
  return (int64_t)sizeof(NdItemDev) * (n_items > 0 ? n_items : 1);
}

extern "C" int vx_nifti_decode(const vx_nifti_dec_item* items, int n_items, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !workspace) VX_FAIL(VX_E_NULL, "vx_nifti_decode: null pointer");
  const int64_t need = vx_nifti_decode_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_nifti_decode: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<NdItemDev> di(n_items);
  int64_t blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_nifti_dec_item& it = items[i];
    if (it.ndim < 1 || it.ndim > 7) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: item %d: ndim %d", i, it.ndim);
    int64_t nvox = 1;
    for (int a = 0; a < it.ndim; ++a) {
      if (it.dims[a] < 0) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: item %d: dims[%d]=%d", i, a, it.dims[a]);
      nvox *= it.dims[a];
      if (nvox > ((int64_t)1 << 40)) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: item %d: too many voxels", i);
    }
    const int es = nd_esize(it.code);
    if (!es) VX_FAIL(VX_E_DTYPE, "vx_nifti_decode: item %d: datatype %d", i, it.code);
    if (it.out_dtype != -1 && it.out_dtype != VX_F32 && it.out_dtype != VX_F64)
      VX_FAIL(VX_E_DTYPE, "vx_nifti_decode: item %d: out_dtype %d", i, it.out_dtype);
    if (it.out_dtype == VX_F32 && it.code != 16) VX_FAIL(VX_E_DTYPE, "vx_nifti_decode: item %d: float32 output of datatype %d", i, it.code);
    const int oes = it.out_dtype == VX_F32 ? 4 : it.out_dtype == VX_F64 ? 8 : es;
    if (it.vox_offset < 0 || it.src_n < it.vox_offset + nvox * es)
      VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: item %d: %lld voxels at %lld beyond src_n=%lld", i, (long long)nvox,
              (long long)it.vox_offset, (long long)it.src_n);
    if (it.dst_n < nvox * oes) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: item %d: dst_n=%lld < %lld", i, (long long)it.dst_n, (long long)(nvox * oes));
    if (!it.src || (nvox > 0 && !it.dst)) VX_FAIL(VX_E_NULL, "vx_nifti_decode: item %d: null pointer", i);
    if (((uintptr_t)it.dst) % oes) VX_FAIL(VX_E_ALIGN, "vx_nifti_decode: item %d: dst not aligned to %d bytes", i, oes);
    NdItemDev& d = di[i];
    d.it = it;
    d.block0 = blocks;
    d.nvox = nvox;
    d.esize = es;
    d.out_es = oes;
    d.aligned = ((uintptr_t)(it.src + it.vox_offset)) % es == 0;
    d.tiled = it.ndim == 3 && nvox > 0;
    d.tx = d.tiled ? (it.dims[0] + ND_TILE - 1) / ND_TILE : 0;
    d.tz = d.tiled ? (it.dims[2] + ND_TILE - 1) / ND_TILE : 0;
    blocks += d.tiled ? (int64_t)d.tx * d.tz * it.dims[1] : (nvox + 255) / 256;
  }
  if (blocks > 0x7FFFFFFF) VX_FAIL(VX_E_SHAPE, "vx_nifti_decode: %lld workgroups", (long long)blocks);
  if (blocks == 0) return VX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = vx_upload_table("vx_nifti_decode", "table upload", workspace, di.data(), sizeof(NdItemDev) * n_items, s)) return rc;
  hipLaunchKernelGGL(nifti_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const NdItemDev*)workspace, n_items);
  VX_CHECK_LAUNCH("vx_nifti_decode");
  return VX_OK;
}
