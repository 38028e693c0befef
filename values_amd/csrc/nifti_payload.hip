// NIfTI-1 payloads of the results tree, assembled on the device (values_amd/results.py: save_case_device; the host
// writer it mirrors is results.save_case, the reference's DataCarrier3D.save_data, data_carrier_3D.py:208-371).
//
// One launch writes every file of a case: a table of items, each the 352-byte header (built on the host: nifti.header_bytes)
// followed by the voxels in Fortran order -- element src[x][y][z] (C order) goes to (z * Y + y) * X + x.  For a fixed y that
// is a transpose of the (x, z) plane, so a workgroup takes a 64 x 64 (x, z) tile of one y: the reads run along z, the
// tile goes through LDS and the writes run along x, both coalesced.
//
// The values are those save_case writes, bit for bit:
//   PROB        float64(src[t][c]) / float64(clip(count, 1))          (sm.astype(float64) / np.clip(count, 1, None))
//   MEAN_PROB   (((PROB[0] + PROB[1]) + ...) + PROB[T-1]) / T          (numpy's mean over the outer axis: sequential sum)
//   ARGMAX      first index of the maximum over c of PROB[t][c]; a NaN is the maximum (np.argmax)
//   ARGMAX_MEAN the same over MEAN_PROB
//   COPY        the element as it is (1, 2, 4 or 8 bytes)
// (the Makefile builds with -ffp-contract=off: no fused operations change a rounding)
#include <vector>

#include "common.h"

namespace {

constexpr int NP_TILE = 64;
constexpr int NP_HDR = 352;

struct NpItemDev {
  vx_nifti_item it;
  int64_t tile0;     // first tile of the item in the launch
  int32_t tx, tz;    // tiles along x and z
};

__device__ __forceinline__ double np_load_prob(const vx_nifti_item& it, int t, int c, int64_t vox) {
  const int64_t i = ((int64_t)t * it.C + c) * ((int64_t)it.X * it.Y * it.Z) + vox;
  double v = it.src_dtype == VX_F64 ? reinterpret_cast<const double*>(it.src)[i] : (double)reinterpret_cast<const float*>(it.src)[i];
  if (it.count) {
    double n = it.count[vox];
    n = n < 1.0 ? 1.0 : n;   // np.clip(count, 1, None): a NaN count stays NaN
    v = v / n;
  }
  return v;
}
__device__ __forceinline__ double np_mean_prob(const vx_nifti_item& it, int c, int64_t vox) {
  double s = np_load_prob(it, 0, c, vox);
  for (int t = 1; t < it.T; ++t) s += np_load_prob(it, t, c, vox);
  return s / (double)it.T;
}
// np.argmax: the first maximum; a NaN wins (the first one)
__device__ __forceinline__ bool np_beats(double v, double best) { return v > best || (v != v); }

__device__ uint64_t np_value(const vx_nifti_item& it, int64_t vox) {
  switch (it.kind) {
    case VX_NIFTI_COPY:
      switch (it.esize) {
        case 1: return reinterpret_cast<const uint8_t*>(it.src)[vox];
        case 2: return reinterpret_cast<const uint16_t*>(it.src)[vox];
        case 4: return reinterpret_cast<const uint32_t*>(it.src)[vox];
        default: return reinterpret_cast<const uint64_t*>(it.src)[vox];
      }
    case VX_NIFTI_PROB: return (uint64_t)__double_as_longlong(np_load_prob(it, it.t, it.c, vox));
    case VX_NIFTI_MEAN_PROB: return (uint64_t)__double_as_longlong(np_mean_prob(it, it.c, vox));
    default: {
      const bool mean = it.kind == VX_NIFTI_ARGMAX_MEAN;
      double best = mean ? np_mean_prob(it, 0, vox) : np_load_prob(it, it.t, 0, vox);
      int idx = 0;
      for (int c = 1; c < it.C && best == best; ++c) {
        const double v = mean ? np_mean_prob(it, c, vox) : np_load_prob(it, it.t, c, vox);
        if (np_beats(v, best)) { best = v; idx = c; }
      }
      return (uint64_t)idx;
    }
  }
}

__device__ __forceinline__ int np_out_esize(const vx_nifti_item& it) {
  return it.kind == VX_NIFTI_COPY ? it.esize : (it.kind == VX_NIFTI_PROB || it.kind == VX_NIFTI_MEAN_PROB) ? 8 : 1;
}

__global__ __launch_bounds__(256) void nifti_payload_kernel(const NpItemDev* __restrict__ items, int n_items, uint8_t* __restrict__ dst) {
  __shared__ uint64_t tile[NP_TILE][NP_TILE + 1];
  const int tid = threadIdx.x;
  // the item of this tile: last item whose first tile is <= blockIdx.x
  int lo = 0, hi = n_items - 1;
  const int64_t b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].tile0 <= b) lo = mid;
    else hi = mid - 1;
  }
  const NpItemDev& d = items[lo];
  const vx_nifti_item& it = d.it;
  const int64_t k = b - d.tile0;
  const int zt = (int)(k % d.tz);
  const int xt = (int)((k / d.tz) % d.tx);
  const int y = (int)(k / ((int64_t)d.tz * d.tx));
  uint8_t* out = dst + it.dst_off;
  if (k == 0 && tid < NP_HDR / 4)
    reinterpret_cast<uint32_t*>(out)[tid] = reinterpret_cast<const uint32_t*>(it.header)[tid];
  const int X = it.X, Y = it.Y, Z = it.Z;
  if ((int64_t)X * Y * Z == 0) return;
  const int x0 = xt * NP_TILE, z0 = zt * NP_TILE;
  // read along z
  {
    const int zz = tid & 63, z = z0 + zz;
    for (int xx = tid >> 6; xx < NP_TILE; xx += 4) {
      const int x = x0 + xx;
      if (x < X && z < Z) tile[xx][zz] = np_value(it, ((int64_t)x * Y + y) * Z + z);
    }
  }
  __syncthreads();
  // write along x
  const int es = np_out_esize(it);
  uint8_t* vox = out + NP_HDR;
  {
    const int xx = tid & 63, x = x0 + xx;
    for (int zz = tid >> 6; zz < NP_TILE; zz += 4) {
      const int z = z0 + zz;
      if (x >= X || z >= Z) continue;
      const uint64_t v = tile[xx][zz];
      const int64_t o = ((int64_t)z * Y + y) * X + x;
      switch (es) {
        case 1: vox[o] = (uint8_t)v; break;
        case 2: reinterpret_cast<uint16_t*>(vox)[o] = (uint16_t)v; break;
        case 4: reinterpret_cast<uint32_t*>(vox)[o] = (uint32_t)v; break;
        default: reinterpret_cast<uint64_t*>(vox)[o] = v; break;
      }
    }
  }
}

int64_t np_payload_bytes(const vx_nifti_item& it) {
  const int es = it.kind == VX_NIFTI_COPY ? it.esize : (it.kind == VX_NIFTI_PROB || it.kind == VX_NIFTI_MEAN_PROB) ? 8 : 1;
  return NP_HDR + (int64_t)it.X * it.Y * it.Z * es;
}

}  // namespace

extern "C" int64_t vx_nifti_payload_bytes(const vx_nifti_item* item) {
  if (!item) return -1;
  return np_payload_bytes(*item);
}

extern "C" size_t vx_nifti_workspace_bytes(int n_items) { return n_items > 0 ? sizeof(NpItemDev) * (size_t)n_items : 0; }

extern "C" int vx_nifti_payload(const vx_nifti_item* items, int n_items, uint8_t* dst, int64_t dst_bytes, void* workspace,
                                size_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !dst || !workspace) VX_FAIL(VX_E_NULL, "vx_nifti_payload: null pointer");
  if (!vx_aligned16(dst)) VX_FAIL(VX_E_ALIGN, "vx_nifti_payload: dst not 16-byte aligned");
  std::vector<NpItemDev> di(n_items);
  int64_t tiles = 0;
  for (int i = 0; i < n_items; ++i) {
    const vx_nifti_item& it = items[i];
    if (it.kind < VX_NIFTI_COPY || it.kind > VX_NIFTI_ARGMAX_MEAN) VX_FAIL(VX_E_DTYPE, "vx_nifti_payload: item %d: kind %d", i, it.kind);
    if (it.X < 0 || it.Y < 0 || it.Z < 0) VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: item %d: shape %d x %d x %d", i, it.X, it.Y, it.Z);
    const int64_t nvox = (int64_t)it.X * it.Y * it.Z;
    if (it.dst_off < 0 || (it.dst_off & 15)) VX_FAIL(VX_E_ALIGN, "vx_nifti_payload: item %d: dst_off %lld (multiple of 16)", i, (long long)it.dst_off);
    if (it.dst_off + np_payload_bytes(it) > dst_bytes)
      VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: item %d: payload [%lld, +%lld) beyond dst_bytes=%lld", i, (long long)it.dst_off,
              (long long)np_payload_bytes(it), (long long)dst_bytes);
    if (it.kind == VX_NIFTI_COPY) {
      if (it.esize != 1 && it.esize != 2 && it.esize != 4 && it.esize != 8) VX_FAIL(VX_E_DTYPE, "vx_nifti_payload: item %d: esize %d", i, it.esize);
    } else {
      if (it.src_dtype != VX_F32 && it.src_dtype != VX_F64) VX_FAIL(VX_E_DTYPE, "vx_nifti_payload: item %d: src_dtype %d", i, it.src_dtype);
      if (it.T < 1 || it.C < 1 || it.t < 0 || it.t >= it.T || it.c < 0 || it.c >= it.C)
        VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: item %d: T=%d C=%d t=%d c=%d", i, it.T, it.C, it.t, it.c);
      if (it.C > 255 && (it.kind == VX_NIFTI_ARGMAX || it.kind == VX_NIFTI_ARGMAX_MEAN))
        VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: item %d: C=%d does not fit uint8 labels", i, it.C);
    }
    if (nvox > 0 && !it.src) VX_FAIL(VX_E_NULL, "vx_nifti_payload: item %d: null source", i);
    di[i].it = it;
    di[i].tile0 = tiles;
    di[i].tx = it.X > 0 ? (it.X + NP_TILE - 1) / NP_TILE : 1;
    di[i].tz = it.Z > 0 ? (it.Z + NP_TILE - 1) / NP_TILE : 1;
    tiles += (int64_t)di[i].tx * di[i].tz * (it.Y > 0 ? it.Y : 1);
  }
  if (tiles > 0x7FFFFFFF) VX_FAIL(VX_E_SHAPE, "vx_nifti_payload: %lld tiles", (long long)tiles);
  const size_t need = sizeof(NpItemDev) * n_items;
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_nifti_payload: workspace %zu < %zu bytes", ws_bytes, need);
  NpItemDev* d_items = (NpItemDev*)workspace;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = vx_upload_table("vx_nifti_payload", "table upload", d_items, di.data(), need, s)) return rc;
  hipLaunchKernelGGL(nifti_payload_kernel, dim3((unsigned)tiles), dim3(256), 0, s, d_items, n_items, dst);
  VX_CHECK_LAUNCH("vx_nifti_payload");
  return VX_OK;
}
