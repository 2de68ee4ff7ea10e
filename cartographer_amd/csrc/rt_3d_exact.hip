// Real-time 3D matcher: the reference's own arithmetic (ScoreCandidate, SM3/
// real_time_correlative_scan_matcher_3d.cc:97-114) on the padded f32 probability brick -- every
// candidate (the exhaustive search) or the finalists the bounds search leaves.  rt_3d.hip has the
// parity notes.
#include <algorithm>

#include "rt_3d_internal.h"

namespace cmx {
namespace {

// uint16 voxel value -> probability in the padded f32 brick, from the voxel list ...

__global__ void FillFloatKernel(float* __restrict__ out, size_t n, float value) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = value;
}

__global__ void ScatterProbabilitiesKernel(const cmx_voxel* __restrict__ voxels, long long n,
                                           PaddedBrick b, float* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cmx_voxel v = voxels[i];
  const size_t off = (static_cast<size_t>(v.z - b.lo_z + 1) * (b.ny + 2) + (v.y - b.lo_y + 1)) *
                         (b.nx + 2) + (v.x - b.lo_x + 1);
  out[off] = ValueToProbabilityDev(v.value);
}

// ... or from a HybridGrid that already lives in HBM as a dense uint16 brick (cmx_grid3d): one
// thread per cell of that brick.
__global__ void BrickProbabilitiesKernel(const uint16_t* __restrict__ cells, long long n, int nx,
                                         int ny, PaddedBrick b, float* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned value = cells[i];
  if (value == 0) return;
  const int x = static_cast<int>(i % nx), y = static_cast<int>((i / nx) % ny),
            z = static_cast<int>(i / (static_cast<long long>(nx) * ny));
  out[(static_cast<size_t>(z + 1) * (b.ny + 2) + (y + 1)) * (b.nx + 2) + (x + 1)] =
      ValueToProbabilityDev(value);
}

// One wavefront = 64 translations of one rotation.  Each lane rotates one point of the
// next 64-point chunk into LDS (the rotation is wave-uniform, so this removes the 64x
// redundant rotation), then all lanes walk the chunk in point order: broadcast LDS read,
// add the lane's translation, cell index, one gather from the padded brick, and the
// reference's sequential f32 accumulation.
__global__ void __launch_bounds__(64)
Rt3DScoreKernel(Rt3DParams P, const float* __restrict__ xyz, int n,
                float* __restrict__ unweighted, float* __restrict__ weighted,
                unsigned* __restrict__ max_bits) {
  __shared__ float4 rotated[64];
  const int lane = threadIdx.x;
  const int t = blockIdx.x * 64 + lane;
  const int r = blockIdx.y;
  const bool valid = t < P.num_translations;
  const float4 q4 = P.rotation[r];
  const Quat q{q4.w, q4.x, q4.y, q4.z};
  const float4 tr = P.translation[valid ? t : 0];
  const float res = P.resolution, inv = P.inv_resolution;
  const int sx = P.grid.nx + 2, sy = P.grid.ny + 2;
  const int ox = 1 - P.grid.lo_x, oy = 1 - P.grid.lo_y, oz = 1 - P.grid.lo_z;
  const int mx = P.grid.nx + 1, my = P.grid.ny + 1, mz = P.grid.nz + 1;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(P.grid.cells), 0, sx * sy * (P.grid.nz + 2) * 4, 0x00020000);

  const auto cell_offset = [&](const float4& rp) -> int {
    const float cx = rp.x + tr.x, cy = rp.y + tr.y, cz = rp.z + tr.z;   // rigid * point
    bool ok = true;
    int ix = FastCellIndex(cx, inv, &ok);
    int iy = FastCellIndex(cy, inv, &ok);
    int iz = FastCellIndex(cz, inv, &ok);
    if (!ok) {
      const int3 idx = CellIndex3(F3{cx, cy, cz}, res);
      ix = idx.x; iy = idx.y; iz = idx.z;
    }
    ix = min(max(ix + ox, 0), mx);
    iy = min(max(iy + oy, 0), my);
    iz = min(max(iz + oz, 0), mz);
    return ((iz * sy + iy) * sx + ix) * 4;
  };

  float acc = 0.f;
  constexpr int kBatch = 8;
  for (int base = 0; base < n; base += 64) {
    const int cnt = min(64, n - base);
    __syncthreads();                       // previous chunk fully consumed
    if (lane < cnt) {
      const int i = base + lane;
      const F3 rp = Rotate(q, F3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
      rotated[lane] = make_float4(rp.x, rp.y, rp.z, 0.f);
    }
    __syncthreads();
    int j = 0;
    for (; j + kBatch <= cnt; j += kBatch) {
      float v[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k)
        v[k] = __uint_as_float(
            __builtin_amdgcn_raw_buffer_load_b32(rsrc, cell_offset(rotated[j + k]), 0, 0));
#pragma unroll
      for (int k = 0; k < kBatch; ++k) acc += v[k];
    }
    for (; j < cnt; ++j)
      acc += __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rsrc, cell_offset(rotated[j]), 0, 0));
  }

  float w = 0.f;
  if (valid) {
    acc /= static_cast<float>(n);
    // Candidate order of the reference: z, y, x, rz, ry, rx nesting.
    const size_t c = static_cast<size_t>(t) * P.num_rotations + r;
    unweighted[c] = acc;
    const double penalty = static_cast<double>(tr.w) * P.wt +
                           static_cast<double>(P.rotation_angle[r]) * P.wr;
    w = static_cast<float>(static_cast<double>(acc) * exp(-(penalty * penalty)));
    weighted[c] = w;
  }
  unsigned bits = __float_as_uint(w);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if (threadIdx.x == 0) atomicMax(max_bits, bits);
}

__global__ void Rt3DCollectKernel(const float* __restrict__ weighted, long long num_candidates,
                                  const unsigned* __restrict__ max_bits, int* __restrict__ count,
                                  long long* __restrict__ finalists, int capacity) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= num_candidates) return;
  const float threshold = __uint_as_float(*max_bits) * (1.f - 1e-5f);
  if (weighted[c] >= threshold) {
    const int slot = atomicAdd(count, 1);
    if (slot < capacity) finalists[slot] = c;
  }
}

// Candidates whose weighted upper bound reaches the best weighted lower bound; `finalists`
// holds r * T + t (the bulk layout), unordered.  Candidates never scored have upper == 0.
__global__ void Rt3DBulkCollectKernel(const float* __restrict__ upper, long long num_candidates,
                                      const unsigned* __restrict__ max_lower_bits,
                                      int* __restrict__ count, int* __restrict__ finalists,
                                      int capacity) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= num_candidates) return;
  if (upper[c] >= __uint_as_float(*max_lower_bits)) {
    const int slot = atomicAdd(count, 1);
    if (slot < capacity) finalists[slot] = static_cast<int>(c);
  }
}

// One block per finalist: the reference's own arithmetic (Rotate, + translation, lround of the
// IEEE quotient, padded f32 probability brick).  The N lookups of a candidate are independent,
// its f32 sum is a chain: waves 1..3 fetch the next 4096 probabilities into one LDS buffer while
// lane 0 of wave 0 runs the chain over the other (ChainSumLds, cmx_device.h).
constexpr int kExact3DChunk = 4096;
__global__ void __launch_bounds__(256)
Rt3DExactKernel(Rt3DParams P, const float* __restrict__ xyz, int n,
                const int* __restrict__ finalists, const int* __restrict__ count, int capacity,
                float* __restrict__ exact) {
  __shared__ __attribute__((aligned(16))) float prob[2][kExact3DChunk];
  const int f = blockIdx.x;
  if (f >= min(*count, capacity)) return;
  const int c = finalists[f];
  const int r = c / P.num_translations, t = c - r * P.num_translations;
  const float4 q4 = P.rotation[r];
  const Quat q{q4.w, q4.x, q4.y, q4.z};
  const float4 tr = P.translation[t];
  const float res = P.resolution;
  const int sx = P.grid.nx + 2, sy = P.grid.ny + 2;
  const int ox = 1 - P.grid.lo_x, oy = 1 - P.grid.lo_y, oz = 1 - P.grid.lo_z;
  const int mx = P.grid.nx + 1, my = P.grid.ny + 1, mz = P.grid.nz + 1;
  const auto fetch = [&](int base, float* out, int first, int stride) {
    const int cnt = min(kExact3DChunk, n - base);
    for (int j = first; j < cnt; j += stride) {
      const int i = base + j;
      const F3 rp = Rotate(q, F3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
      const int3 idx = CellIndex3(F3{rp.x + tr.x, rp.y + tr.y, rp.z + tr.z}, res);
      const int ix = min(max(idx.x + ox, 0), mx);
      const int iy = min(max(idx.y + oy, 0), my);
      const int iz = min(max(idx.z + oz, 0), mz);
      out[j] = P.grid.cells[(static_cast<size_t>(iz) * sy + iy) * sx + ix];
    }
    // (the chain runs over whole banks of 64: + 0 leaves the non-negative sum as it is)
    for (int j = cnt + first; j < ((cnt + 63) & ~63); j += stride) out[j] = 0.f;
  };
  float acc = 0.f;
  fetch(0, prob[0], threadIdx.x, blockDim.x);
  __syncthreads();
  int b = 0;
  for (int base = 0; base < n; base += kExact3DChunk, b ^= 1) {
    if (threadIdx.x >= 64) {
      if (base + kExact3DChunk < n) fetch(base + kExact3DChunk, prob[b ^ 1], threadIdx.x - 64,
                                          blockDim.x - 64);
    } else if (threadIdx.x == 0) {
      const int cnt = min(kExact3DChunk, n - base);
      acc = ChainSumLds(prob[b], (cnt + 63) & ~63, acc);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) exact[f] = acc / static_cast<float>(n);
}

}  // namespace

void BuildProbabilityBrick(Workspace& ws, const Rt3DGridSource& grid, Rt3DDevice* D) {
  const Brick* resident = grid.resident;
  const int64_t num_voxels = grid.num_voxels;
  const PaddedBrick& box = D->brick;
  const size_t cells = static_cast<size_t>(box.nx + 2) * (box.ny + 2) * (box.nz + 2);
  float* d_cells = ws.dev[kSlotProbabilities].ReserveAs<float>(cells);
  D->brick.cells = d_cells;
  FillFloatKernel<<<DivUp(cells, 256), 256, 0, ws.stream>>>(d_cells, cells, 0.1f);
  if (resident != nullptr) {
    const long long count = static_cast<long long>(resident->nx) * resident->ny * resident->nz;
    BrickProbabilitiesKernel<<<DivUp(count, 256), 256, 0, ws.stream>>>(
        static_cast<const uint16_t*>(resident->cells), count, resident->nx, resident->ny,
        D->brick, d_cells);
  } else if (num_voxels > 0) {
    D->d_vox = UploadVoxels(ws, grid.voxels, num_voxels);
    ScatterProbabilitiesKernel<<<DivUp(num_voxels, 256), 256, 0, ws.stream>>>(
        D->d_vox, num_voxels, D->brick, d_cells);
  }
  CMX_HIP(hipGetLastError());
}

void RunExhaustiveSearch(Workspace& ws, const Rt3DSearchSpace& S, const Rt3DDevice& D,
                         Rt3DFinalists* out) {
  const long long num_candidates = S.num_candidates;
  Rt3DExhaustiveMisc* d_misc = D.d_misc;
  RecordEvent(ws.ev_k0, ws.stream);
  Rt3DScoreKernel<<<dim3(DivUp(S.T, 64), static_cast<unsigned>(S.R)), 64, 0, ws.stream>>>(
      D.P, D.d_xyz, S.n, D.d_unweighted, D.d_weighted, &d_misc->max_bits);
  RecordEvent(ws.ev_k1, ws.stream);
  Rt3DCollectKernel<<<DivUp(num_candidates, 256), 256, 0, ws.stream>>>(
      D.d_weighted, num_candidates, &d_misc->max_bits, &d_misc->count, d_misc->finalists,
      kFinalistCap);
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_end, ws.stream);
  const Rt3DExhaustiveMisc& h_misc = D.pinned->exhaustive;
  CMX_HIP(hipMemcpyAsync(&D.pinned->exhaustive, d_misc, sizeof(Rt3DExhaustiveMisc),
                         hipMemcpyDeviceToHost, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));
  const int count = h_misc.count;
  if (count <= kFinalistCap) {
    out->index.assign(h_misc.finalists, h_misc.finalists + count);
    std::sort(out->index.begin(), out->index.end());
    out->acc.resize(count);
    for (int i = 0; i < count; ++i)
      CMX_HIP(hipMemcpy(&out->acc[i], D.d_unweighted + out->index[i], sizeof(float),
                        hipMemcpyDeviceToHost));
  } else {
    out->index.resize(num_candidates);
    for (long long c = 0; c < num_candidates; ++c) out->index[c] = c;
    out->acc.resize(num_candidates);
    CMX_HIP(hipMemcpy(out->acc.data(), D.d_unweighted, sizeof(float) * num_candidates,
                      hipMemcpyDeviceToHost));
  }
}

void CollectAndScoreFinalists(Rt3DBoundsSearch* run) {
  const Rt3DSearchSpace& S = *run->S;
  Rt3DBulkHead* d_head = run->d_head;
  Rt3DBulkCollectKernel<<<DivUp(S.num_candidates, 256), 256, 0, run->stream()>>>(
      run->d_upper, S.num_candidates, &d_head->max_lower, &d_head->count, d_head->finalists,
      kBulkFinalistCap);
  Rt3DExactKernel<<<kBulkFinalistCap, 256, 0, run->stream()>>>(
      run->D->P, run->D->d_xyz, S.n, d_head->finalists, &d_head->count, kBulkFinalistCap,
      d_head->exact);
}

}  // namespace cmx
