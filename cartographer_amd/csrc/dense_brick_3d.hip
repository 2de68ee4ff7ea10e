// Dense device bricks from voxel lists: the helpers scan_matching_3d.h declares for every 3D
// matcher (fast_3d_stack.hip, fast_3d_stack_batch.hip, ceres_3d.hip and the real-time matcher,
// rt_3d.hip and rt_3d_exact.hip).
#include <algorithm>

#include "scan_matching_3d.h"

namespace cmx {
namespace {

// Workspace::dev slot of the voxel upload.  The callers lease workspaces whose other slots their
// own units index by number (Rt3DSlot, rt_3d_internal.h, lists this one as kSlotVoxels).
constexpr int kSlotVoxelUpload = 15;

__global__ void ScatterVoxelsKernel(const cmx_voxel* __restrict__ voxels, long long n, Brick b,
                                    int bytes_per_cell) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ScatterVoxel(voxels[i], b, bytes_per_cell);
}

}  // namespace

Brick BoxBrick(const int lo[3], const int hi[3]) {
  for (int k = 0; k < 3; ++k) {
    CMX_REQUIRE(lo[k] > -(1 << 20) && hi[k] < (1 << 20), "voxel index out of range");
  }
  Brick b{};
  b.lo_x = lo[0]; b.lo_y = lo[1]; b.lo_z = lo[2];
  b.nx = hi[0] - lo[0] + 1; b.ny = hi[1] - lo[1] + 1; b.nz = hi[2] - lo[2] + 1;
  return b;
}

cmx_voxel* UploadVoxels(Workspace& ws, const cmx_voxel* voxels, int64_t n) {
  cmx_voxel* d_vox = ws.dev[kSlotVoxelUpload].ReserveAs<cmx_voxel>(n);
  CMX_HIP(hipMemcpyAsync(d_vox, voxels, n * sizeof(cmx_voxel), hipMemcpyHostToDevice, ws.stream));
  return d_vox;
}

void VoxelBoxOrOrigin(const cmx_voxel* voxels, int64_t n, int lo[3], int hi[3]) {
  if (VoxelBounds(voxels, n, lo, hi)) return;
  lo[0] = lo[1] = lo[2] = 0;
  hi[0] = hi[1] = hi[2] = 0;
}

bool VoxelBounds(const cmx_voxel* voxels, int64_t n, int lo[3], int hi[3]) {
  if (n <= 0) return false;
  // The running box stays in locals: the callers are in other files, and through `lo` and `hi`
  // (which may point into the list, for all the compiler knows) every step is a store and a
  // load -- twice the time on a real-time match's 95 k voxels.
  int lx = voxels[0].x, ly = voxels[0].y, lz = voxels[0].z, hx = lx, hy = ly, hz = lz;
  for (int64_t i = 1; i < n; ++i) {
    lx = std::min(lx, voxels[i].x); hx = std::max(hx, voxels[i].x);
    ly = std::min(ly, voxels[i].y); hy = std::max(hy, voxels[i].y);
    lz = std::min(lz, voxels[i].z); hz = std::max(hz, voxels[i].z);
  }
  lo[0] = lx; lo[1] = ly; lo[2] = lz;
  hi[0] = hx; hi[1] = hy; hi[2] = hz;
  return true;
}

int GridSizeOf(const cmx_voxel* voxels, int64_t n) {
  int gs = 128;
  int lo[3], hi[3];
  if (!VoxelBounds(voxels, n, lo, hi)) return gs;
  auto fits = [&](int g) {
    const int h = g / 2;
    for (int k = 0; k < 3; ++k)
      if (lo[k] < -h || hi[k] >= h) return false;
    return true;
  };
  while (!fits(gs)) gs *= 2;
  return gs;
}

Brick DenseBrickGeometry(const int lo[3], const int hi[3], int bytes_per_cell, size_t* bytes) {
  const Brick b = BoxBrick(lo, hi);
  const size_t cells = static_cast<size_t>(b.nx) * b.ny * b.nz;
  CMX_REQUIRE(cells * bytes_per_cell < (size_t(8) << 30),
              "dense grid of %d x %d x %d cells is too large", b.nx, b.ny, b.nz);
  *bytes = cells * bytes_per_cell;
  return b;
}

void AllocateDenseBrick(const int lo[3], const int hi[3], int bytes_per_cell, DeviceBrick* out) {
  Brick b = DenseBrickGeometry(lo, hi, bytes_per_cell, &out->bytes);
  CMX_HIP(hipMalloc(&out->mem, out->bytes + 16));   // (+16: aligned 8-byte reads of the last cells)
  b.cells = out->mem;
  out->desc = b;
}

void BuildBrickFromVoxels(Workspace& ws, const cmx_voxel* voxels, int64_t n, int bytes_per_cell,
                          DeviceBrick* out) {
  int lo[3], hi[3];
  VoxelBoxOrOrigin(voxels, n, lo, hi);
  AllocateDenseBrick(lo, hi, bytes_per_cell, out);
  const Brick b = out->desc;
  CMX_HIP(hipMemsetAsync(out->mem, 0, out->bytes, ws.stream));
  if (n > 0) {
    const cmx_voxel* d_vox = UploadVoxels(ws, voxels, n);
    ScatterVoxelsKernel<<<DivUp(n, 256), 256, 0, ws.stream>>>(d_vox, n, b, bytes_per_cell);
    CMX_HIP(hipGetLastError());
  }
  CMX_HIP(hipStreamSynchronize(ws.stream));   // `voxels` is borrowed host memory
}

}  // namespace cmx
