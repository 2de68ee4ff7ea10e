// Real-time 3D matcher: integer bounds (rotation blocks, groups of translations, then single
// candidates) that select the finalists rt_3d_exact.hip scores exactly.
//
// The reference's score of a candidate is mean_p P(cell(T_c p)) summed in f32 in point order
// (:97-114), and P is affine in the stored value: P = kMin + u * kScale with
// u = max(value, 1) - 1 (0 for unknown / outside; real arithmetic -- the f32 table rounds each
// entry by < 1.2e-7).  Integer sums of u are exact and order-free, so most of the search
// needs neither the f32 chain nor the IEEE divisions of GetCellIndex, and most candidates
// need not be scored at all:
//   * the grid becomes a padded uint8 brick q = u >> 7 with a zero halo as wide as twice the
//     reach of the translation window; rotated points are clamped (while they are staged) to
//     one reach outside the stored box, so no lookup needs a bounds test;
//   * GROUP pass: the (2L+1)^3 translations are tiled by 2 x 2 x 2 blocks of lattice steps.
//     The members of a block lie within 0.87 cells (per axis) of its centre, so the cell any
//     member reads is the centre's cell or one of its 26 neighbours: one lookup of the centre
//     in the 3 x 3 x 3-dilated brick bounds all eight members from above (the branch-and-bound
//     idea of the fast matcher, one level deep).  1/6 of the lookups, no exactness needed;
//   * CANDIDATE pass, only for the members of groups whose weighted upper bound reaches the
//     best weighted lower bound known: the cell index is rint(fma(c, RN(1/res), pad - lo))
//     with c = rp + tr exactly the reference's f32 coordinate; it equals the reference's
//     lround(c / res) unless the quotient lies within `1/2 - guard` of a half-integer.  Such
//     lookups are not repaired but COUNTED (per four points): each moves the sum by at most
//     255, which widens the candidate's score interval instead of costing a slow path.
//     Per candidate this yields Q and A with sum(u) in [128 (Q - 1020 A), 128 (Q + 1020 A) +
//     127 N], i.e. an interval for the f32 score once the rounding of the N-term f32 chain
//     ((N + 8) 2^-24, relative) is added;
//   * every candidate whose weighted upper bound reaches the best weighted lower bound is a
//     finalist; Rt3DExactKernel recomputes those with the reference's own arithmetic, and
//     the host applies the libm weight and the first-maximum rule to them exactly as before.
// Returned score and pose are bit-identical to the one-thread-per-candidate kernel
// (Rt3DScoreKernel), which remains the path for flat score landscapes (more finalists than the
// list holds) and for windows / grids beyond the limits checked in ModeOf (Rt3DMode::use_bulk).
//
// The sums of the group and candidate passes come from the gather kernel below or, identically,
// from the LDS tiles of rt_3d_tiles.hip; this unit decides which runs, sizes the launches from
// the read-backs and, with the debug switch rt3d_crosscheck, compares the two.
#include <algorithm>
#include <cstring>

#include "rt_3d_internal.h"

namespace cmx {
namespace {

// uint16 voxel value -> q = (max(value & 32767, 1) - 1) >> 7 in the padded bricks: row-major
// (to be dilated for the group pass) and tiled (candidate pass).
__global__ void ScatterBulkKernel(const cmx_voxel* __restrict__ voxels, long long n, int lo_x,
                                  int lo_y, int lo_z, int pad, int px, int py, int tiles_y,
                                  int pitch_z, uint8_t* __restrict__ rows,
                                  uint8_t* __restrict__ tiled) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const cmx_voxel v = voxels[i];
  const unsigned x = v.x - lo_x + pad, y = v.y - lo_y + pad, z = v.z - lo_z + pad;
  const unsigned value = v.value & 32767u;
  const uint8_t q = static_cast<uint8_t>((max(value, 1u) - 1u) >> 7);
  rows[(static_cast<size_t>(z) * py + y) * px + x] = q;
  tiled[TiledOffset(x, y, z, tiles_y, pitch_z)] = q;
}

// The same conversion from a HybridGrid that already lives in HBM as a dense uint16 brick
// (cmx_grid3d): one thread per cell of that brick.
__global__ void BrickBulkKernel(const uint16_t* __restrict__ cells, long long n, int nx, int ny,
                                int pad, int px, int py, int tiles_y, int pitch_z,
                                uint8_t* __restrict__ rows, uint8_t* __restrict__ tiled) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned raw = cells[i];
  if (raw == 0) return;
  const unsigned x = static_cast<unsigned>(i % nx) + pad,
                 y = static_cast<unsigned>((i / nx) % ny) + pad,
                 z = static_cast<unsigned>(i / (static_cast<long long>(nx) * ny)) + pad;
  const unsigned value = raw & 32767u;
  const uint8_t q = static_cast<uint8_t>((max(value, 1u) - 1u) >> 7);
  rows[(static_cast<size_t>(z) * py + y) * px + x] = q;
  tiled[TiledOffset(x, y, z, tiles_y, pitch_z)] = q;
}

// 3 x 3 x 3 dilation of the padded brick in two passes (x, then y and z).  The halo is wider
// than one cell, so clamped neighbours at the array border read zeros like the cell itself.
__global__ void DilateXKernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int px,
                              size_t cells) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= cells) return;
  const int x = static_cast<int>(i % px);
  unsigned v = in[i];
  if (x > 0) v = max(v, static_cast<unsigned>(in[i - 1]));
  if (x + 1 < px) v = max(v, static_cast<unsigned>(in[i + 1]));
  out[i] = static_cast<uint8_t>(v);
}
__global__ void DilateYZKernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int px,
                               int py, int pz) {
  const size_t cells = static_cast<size_t>(px) * py * pz;
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= cells) return;
  const int x = static_cast<int>(i % px);
  const int y = static_cast<int>((i / px) % py);
  const int z = static_cast<int>(i / (static_cast<size_t>(px) * py));
  unsigned v = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = min(max(y + dy, 0), py - 1), zz = min(max(z + dz, 0), pz - 1);
      v = max(v, static_cast<unsigned>(in[(static_cast<size_t>(zz) * py + yy) * px + x]));
    }
  out[i] = static_cast<uint8_t>(v);
}

// Group pass: grid (ceil(R G / 256)); candidate pass: grid (work descriptors, 1, point
// slices).  256 threads: wave w of a block owns work items 256 chunk + 64 w .. + 63.  kGroups: group pass (no ambiguity bookkeeping, upper
// bounds only, all points in one block).  Candidate pass: the work lists are short, so the
// points are split over blockIdx.z as well and (Q, A) are accumulated with atomics (integer
// sums are order-free); Rt3DBoundsKernel turns them into bounds.
template <bool kGroups>
__global__ void __launch_bounds__(kBulk3DThreads)
Rt3DBulkKernel(Rt3DBulkParams P, const float* __restrict__ xyz) {
  // Points 2p, 2p + 1 as {x0, x1, y0, y1, z0, z1}: what the packed f32 instructions read.
  // Group pass: a block's 256 lanes are a window of the flat (rotation, group) sequence, i.e.
  // they belong to one or two consecutive rotations (G groups fill 3.4 wavefronts: a block per
  // rotation left 16 % of the lanes idle); both rotations' points are staged.
  __shared__ v2f stage[2][kGroups ? 2 : 1][3 * kBulk3DChunk / 2];
  const int tid = threadIdx.x;
  int r, t, rotation_a = 0;
  bool valid, wave_active;
  if (kGroups && gridDim.y > 1) {
    // (few groups per rotation, G < 128: a block would span more than two rotations; one
    // rotation per blockIdx.y then, as the candidate pass)
    r = blockIdx.y;
    if (r >= P.num_rotations) return;                // (grid.y is at least 2 to mark this mode)
    t = min(static_cast<int>(blockIdx.x * kBulk3DThreads + tid), P.num_translations - 1);
    valid = static_cast<int>(blockIdx.x * kBulk3DThreads + tid) < P.num_translations;
    wave_active = static_cast<int>(blockIdx.x * kBulk3DThreads + (tid & ~63)) < P.num_translations;
    rotation_a = r;
  } else if (kGroups) {
    // blockDim.x <= G + 1 lanes: they belong to at most two consecutive rotations.
    const long long first_flat = static_cast<long long>(blockIdx.x) * blockDim.x;
    const long long flat = first_flat + tid;
    const long long total = static_cast<long long>(P.num_rotations) * P.num_translations;
    rotation_a = static_cast<int>(first_flat / P.num_translations);
    valid = flat < total;
    const long long f = valid ? flat : total - 1;
    r = static_cast<int>(f / P.num_translations);
    t = static_cast<int>(f - static_cast<long long>(r) * P.num_translations);
    wave_active = first_flat + (tid & ~63) < total;
  } else {
    const int2 work = P.blocks[blockIdx.x];
    r = work.x;                                      // (this kernel: lists of one rotation)
    const int slot = work.y * P.block_items + tid;
    const int count = P.counts[r];
    if (work.y * P.block_items >= count) return;                         // whole block idle
    wave_active = work.y * P.block_items + (tid & ~63) < count;
    valid = slot < count;
    t = P.items[static_cast<size_t>(r) * P.num_translations + (valid ? slot : count - 1)];
    rotation_a = r;
  }
  const int which = r - rotation_a;                  // 0 or 1: which staged rotation a lane reads
  const int rotation_b = min(rotation_a + 1, P.num_rotations - 1);
  const float4 qa4 = P.rotation[rotation_a], qb4 = P.rotation[rotation_b];
  const Quat q{qa4.w, qa4.x, qa4.y, qa4.z}, q_b{qb4.w, qb4.x, qb4.y, qb4.z};
  const float4 tr = P.translation[t];
  const int first = kGroups ? 0 : blockIdx.z * P.slice_points;   // (blockIdx.z: point slice)
  const int n = kGroups ? P.n : min(P.n, first + P.slice_points);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(P.cells), 0, P.cell_count, 0x00020000);

  const auto stage_chunk = [&](int base, int buf) {
    for (int k = tid; k < kBulk3DChunk; k += blockDim.x) {   // (the group pass may run 192 wide)
      const int i = base + k;
#pragma unroll
      for (int w = 0; w < (kGroups ? 2 : 1); ++w) {
        // Padding points sit one reach below the box: every translation reads the zero halo.
        float4 out = make_float4(P.lo_x - P.t0x, P.lo_y - P.t0y, P.lo_z - P.t0z, 0.f);
        if (i < n) {
          const F3 rp = Rotate(w == 0 ? q : q_b, F3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
          out.x = ClampStage(rp.x, P.t0x, P.lo_x, P.hi_x);
          out.y = ClampStage(rp.y, P.t0y, P.lo_y, P.hi_y);
          out.z = ClampStage(rp.z, P.t0z, P.lo_z, P.hi_z);
        }
        float* dst = reinterpret_cast<float*>(stage[buf][w]) + 6 * (k >> 1) + (k & 1);
        dst[0] = out.x; dst[2] = out.y; dst[4] = out.z;
      }
    }
  };

  const v2f trx = {tr.x, tr.x}, try_ = {tr.y, tr.y}, trz = {tr.z, tr.z};
  const v2f inv = {P.inv_resolution, P.inv_resolution};
  const v2f ofx = {P.off_x, P.off_x}, ofy = {P.off_y, P.off_y}, ofz = {P.off_z, P.off_z};
  const v2f px2 = {P.pitch_x, P.pitch_x}, py2 = {P.pitch_y, P.pitch_y};
  const float guard = P.guard;
  unsigned acc = 0, ambiguous = 0;

  stage_chunk(first, 0);
  __syncthreads();
  int buf = 0;
  unsigned p0 = 0, p1 = 0, p2 = 0, p3 = 0;     // the previous four lookups, still in flight
  for (int base = first; base < n; base += kBulk3DChunk, buf ^= 1) {
    if (base + kBulk3DChunk < n) stage_chunk(base + kBulk3DChunk, buf ^ 1);
    if (wave_active) {
      const v2f* __restrict__ s = stage[buf][kGroups ? which : 0];
#pragma unroll 2
      for (int j = 0; j < kBulk3DChunk; j += 4) {
        unsigned v[4];
        float g = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
          const v2f* pr = s + 3 * ((j + k) >> 1);                // LDS broadcast reads
          const v2f cx = pr[0] + trx;                            // rigid * point, as the reference
          const v2f cy = pr[1] + try_;
          const v2f cz = pr[2] + trz;
          const v2f qx = __builtin_elementwise_fma(cx, inv, ofx);
          const v2f qy = __builtin_elementwise_fma(cy, inv, ofy);
          const v2f qz = __builtin_elementwise_fma(cz, inv, ofz);
          const v2f nx = {rintf(qx.x), rintf(qx.y)};
          const v2f ny = {rintf(qy.x), rintf(qy.y)};
          const v2f nz = {rintf(qz.x), rintf(qz.y)};
          if (!kGroups) {
            const v2f dx = qx - nx, dy = qy - ny, dz = qz - nz;
            g = fmaxf(fmaxf(g, fabsf(dx.x)), fabsf(dx.y));
            g = fmaxf(fmaxf(g, fabsf(dy.x)), fabsf(dy.y));
            g = fmaxf(fmaxf(g, fabsf(dz.x)), fabsf(dz.y));
          }
          if (kGroups) {
            // (z * pitch_y + y) * pitch_x + x: integers below 2^24, exact in f32.
            const v2f o =
                __builtin_elementwise_fma(__builtin_elementwise_fma(nz, py2, ny), px2, nx);
            v[k] = __builtin_amdgcn_raw_buffer_load_b8(rsrc, static_cast<unsigned>(o.x), 0, 0);
            v[k + 1] = __builtin_amdgcn_raw_buffer_load_b8(rsrc, static_cast<unsigned>(o.y), 0, 0);
          } else {
            const unsigned o0 = TiledOffset(static_cast<unsigned>(nx.x), static_cast<unsigned>(ny.x),
                                            static_cast<unsigned>(nz.x), P.tiles_y, P.pitch_z);
            const unsigned o1 = TiledOffset(static_cast<unsigned>(nx.y), static_cast<unsigned>(ny.y),
                                            static_cast<unsigned>(nz.y), P.tiles_y, P.pitch_z);
            v[k] = __builtin_amdgcn_raw_buffer_load_b8(rsrc, o0, 0, 0);
            v[k + 1] = __builtin_amdgcn_raw_buffer_load_b8(rsrc, o1, 0, 0);
          }
        }
        if (!kGroups) ambiguous += g > guard ? 1u : 0u;
        acc += (p0 + p1) + (p2 + p3);            // consumed one iteration after they were issued
        p0 = v[0]; p1 = v[1]; p2 = v[2]; p3 = v[3];
      }
    }
    __syncthreads();
  }
  acc += (p0 + p1) + (p2 + p3);

  const size_t c = static_cast<size_t>(r) * P.num_translations + t;
  if (!kGroups) {
    if (valid) {
      atomicAdd(&P.sums[c].x, acc);
      if (ambiguous) atomicAdd(&P.sums[c].y, ambiguous);
    }
    return;
  }
  float lower = 0.f, upper = 0.f;
  if (valid) {
    Bounds3D(P, acc, 0u, tr.w, r, &lower, &upper);
    P.upper[c] = upper;
  }
  // Bounds are positive: bit order == value order.
  unsigned bits = __float_as_uint(upper);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if ((tid & 63) == 0 && bits != 0) atomicMax(P.max_upper_bits, bits);
}

// grid (work descriptors): bounds of the candidates on the work lists from their (Q, A).
__global__ void __launch_bounds__(1024)
Rt3DBoundsKernel(Rt3DBulkParams P) {
  const int2 work = P.blocks[blockIdx.x];
  const int list = work.x;
  const int slot = work.y * P.block_items + threadIdx.x;
  const int count = P.counts[list];
  float lower = 0.f, upper = 0.f;
  if (slot < count) {
    const int entry =
        P.items[static_cast<size_t>(list) * P.list_rotations * P.num_translations + slot];
    const int w = entry / P.num_translations, t = entry - w * P.num_translations;
    const int r = list * P.list_rotations + w;
    const size_t c = static_cast<size_t>(r) * P.num_translations + t;
    const uint2 qa = P.sums[c];
    Bounds3D(P, qa.x, qa.y, P.translation[t].w, r, &lower, &upper);
    P.upper[c] = upper;
  }
  unsigned bits = __float_as_uint(lower);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(P.max_lower_bits, bits);
}

// ---- Staged candidate pass --------------------------------------------------------------
// The second candidate round scores every member of every group the best lower bound cannot
// exclude -- a tenth of C4's 1.77 M candidates, each over all 65 536 points, although all but a
// handful lose by a wide margin: the group bound is loose (a 3 x 3 x 3 dilation), the candidates
// themselves are not close.  But the group bound is a sum over POINTS of values that dominate
// the member's own value point by point, so for any part S of the cloud
//     score sum of c  <=  (sum of c over S)  +  (group sum over the rest),
// and the right-hand side tightens as S grows.  The cloud is cut into three segments (a
// quarter, a quarter, a half: Rt3DBinScanKernel), the group pass reports a group's sum by
// segment, and the round runs segment by segment: after the first and after the second,
// candidates whose weighted bound has fallen below the best lower bound are dropped from the
// work lists (they keep `upper` = 0: never finalists, exactly what their full evaluation would
// have concluded).  C4 (tools/prototype numbers in profiles/HISTORY.md 5.4): of 154 k candidates 48 % are
// alive after a quarter of the points, 10 % after half.
//
// grid (work descriptors): flags[r][t] = 1 for the listed candidates that stay.  `stage` = the
// segment just finished (0 or 1).  Verification mode (`stage_ub` != null: debug switch rt3d_verify): the
// lists stay as they are, every candidate is evaluated in full, and this kernel only records the
// decision (`dropped`) and the smallest bound seen (in units of q) for Rt3DStageCheckKernel.
__global__ void __launch_bounds__(1024)
Rt3DStageFilterKernel(Rt3DBulkParams P, const uint2* __restrict__ group_total,
                      const uint2* __restrict__ group_seg, int num_groups, int side,
                      int groups_per_axis, int stage, uint8_t* __restrict__ flags,
                      unsigned long long* __restrict__ stage_ub, uint8_t* __restrict__ dropped) {
  const int2 work = P.blocks[blockIdx.x];
  const int list = work.x;
  const int slot = work.y * P.block_items + threadIdx.x;
  if (slot >= P.counts[list]) return;
  const int entry =
      P.items[static_cast<size_t>(list) * P.list_rotations * P.num_translations + slot];
  const int w = entry / P.num_translations, t = entry - w * P.num_translations;
  const int r = list * P.list_rotations + w;
  const size_t c = static_cast<size_t>(r) * P.num_translations + t;
  const uint2 qa = P.sums[c];                       // over the segments done so far
  const int x = t % side, y = (t / side) % side, z = t / (side * side);
  const int g = ((z >> 1) * groups_per_axis + (y >> 1)) * groups_per_axis + (x >> 1);
  const size_t gi = static_cast<size_t>(r) * num_groups + g;
  const uint2 seg = group_seg[gi];
  const unsigned long long rest = static_cast<unsigned long long>(group_total[gi].x) - seg.x -
                                  (stage >= 1 ? seg.y : 0u);
  const unsigned long long q_hi = static_cast<unsigned long long>(qa.x) +
                                  static_cast<unsigned long long>(qa.y) * kAmbiguousQuad + rest;
  // Bounds3D's upper bound for an integer sum of q_hi (quantisation, table rounding and the f32
  // chain's slack included), rounded outwards
  const double mean_hi = P.min_probability + P.scale_over_n * static_cast<double>(q_hi) + P.slack_hi;
  const double penalty = static_cast<double>(P.translation[t].w) * P.wt +
                         static_cast<double>(P.rotation_angle[r]) * P.wr;
  const double weight = exp(-(penalty * penalty));
  const float upper = static_cast<float>(mean_hi * weight * (1. + P.delta)) * (1.f + 0x1p-22f);
  const bool stays = upper >= __uint_as_float(*P.max_lower_bits);
  if (stage_ub != nullptr) {
    stage_ub[c] = stage == 0 ? q_hi : min(stage_ub[c], q_hi);
    if (stage == 0) dropped[c] = stays ? 0 : 1;
    else if (!stays) dropped[c] = 1;
    return;
  }
  if (stays) flags[c] = 1;
}

// Verification mode of the staged pass, after the round's bounds: every bound recorded on the way
// must dominate the candidate's own full sum (at its lower end), and a candidate the shipped
// path would have dropped gets the `upper` = 0 it would have kept there.  grid (work descriptors).
__global__ void __launch_bounds__(1024)
Rt3DStageCheckKernel(Rt3DBulkParams P, const unsigned long long* __restrict__ stage_ub,
                     const uint8_t* __restrict__ dropped, int* __restrict__ violations) {
  const int2 work = P.blocks[blockIdx.x];
  const int list = work.x;
  const int slot = work.y * P.block_items + threadIdx.x;
  if (slot >= P.counts[list]) return;
  const int entry =
      P.items[static_cast<size_t>(list) * P.list_rotations * P.num_translations + slot];
  const int w = entry / P.num_translations, t = entry - w * P.num_translations;
  const int r = list * P.list_rotations + w;
  const size_t c = static_cast<size_t>(r) * P.num_translations + t;
  const uint2 qa = P.sums[c];                       // the full sum now
  const unsigned long long spread = static_cast<unsigned long long>(qa.y) * kAmbiguousQuad;
  const unsigned long long q_lo = qa.x > spread ? qa.x - spread : 0ull;
  if (stage_ub[c] < q_lo) atomicAdd(violations, 1);
  if (dropped[c]) {
    if (P.upper[c] >= __uint_as_float(*P.max_lower_bits)) atomicAdd(violations, 1);   // a finalist!
    P.upper[c] = 0.f;
  }
}

// Debug switch rt3d_verify (tests): a group's upper bound must not lie below the LOWER bound of any of
// its members that was scored -- both bracket the same true score.  (A group pass reading the
// wrong staged rotation once produced garbage bounds that every parity test survived: the
// optimum happened not to be pruned.)  grid (work descriptors).
__global__ void __launch_bounds__(1024)
Rt3DVerifyKernel(Rt3DBulkParams P, const float* __restrict__ group_upper, int num_groups,
                 int side, int groups_per_axis, int* __restrict__ violations) {
  const int2 work = P.blocks[blockIdx.x];
  const int list = work.x;
  const int slot = work.y * P.block_items + threadIdx.x;
  if (slot >= P.counts[list]) return;
  const int entry =
      P.items[static_cast<size_t>(list) * P.list_rotations * P.num_translations + slot];
  const int w = entry / P.num_translations, t = entry - w * P.num_translations;
  const int r = list * P.list_rotations + w;
  const uint2 qa = P.sums[static_cast<size_t>(r) * P.num_translations + t];
  float lower, upper;
  Bounds3D(P, qa.x, qa.y, P.translation[t].w, r, &lower, &upper);
  const int x = t % side, y = (t / side) % side, z = t / (side * side);
  const int g = ((z >> 1) * groups_per_axis + (y >> 1)) * groups_per_axis + (x >> 1);
  if (group_upper[static_cast<size_t>(r) * num_groups + g] < lower) atomicAdd(violations, 1);
}

// Group pass of the tiled path: weighted upper bounds from the accumulated sums.
__global__ void Rt3DSumBoundsKernel(Rt3DBulkParams P) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const long long total = static_cast<long long>(P.num_rotations) * P.num_translations;
  float upper = 0.f;
  if (c < total) {
    const int r = static_cast<int>(c / P.num_translations);
    const int t = static_cast<int>(c - static_cast<long long>(r) * P.num_translations);
    float lower;
    Bounds3D(P, P.sums[c].x, 0u, P.translation[t].w, r, &lower, &upper);
    P.upper[c] = upper;
  }
  unsigned bits = __float_as_uint(upper);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(P.max_upper_bits, bits);
}

// ---- the level above the groups: blocks of 2 x 2 x 2 ROTATIONS ----------------------------------
// A rotation block (rb, g) = the rotations of a 2 x 2 x 2 block of the angle-axis lattice x the
// translations of group g, bounded by ONE lookup per point at the block's centre rotation and the
// group's centre translation in the brick dilated TWICE (5 x 5 x 5): a member's rotation vector
// lies within half a step per axis of the centre vector, i.e. within 0.866 steps (x 1.03 for the
// non-commuting part while the window stays below 0.2 rad), a step moves the farthest point by
// one cell (step = 0.999 acos(1 - res^2 / 2 r_max^2)), so the member's rotated point lies within
// 0.89 cells of the centre's, + 0.87 for the translation block + 1/16 for the fixed-point cell:
// 1.82 < 2 cells per axis.  Weight: the smallest member angle and distance.  The (rotation, group)
// pairs of the blocks a threshold cannot exclude then go through the group pass proper
// (Rt3DTileKernel<true, true>, work lists as in the candidate passes); all other pairs keep an
// upper bound of -1: never selected.  As every bound here, these only SELECT what is scored.
//
// pair (r, g) := flagged for the group pass if its block's bound reaches threshold * factor and it
// has not been computed yet.
__global__ void Rt3DSelectPairsKernel(const float* __restrict__ block_upper, int num_groups,
                                      int num_rotations, int side_r, int blocks_per_axis,
                                      const unsigned* __restrict__ threshold_bits, float factor,
                                      uint8_t* __restrict__ computed, uint8_t* __restrict__ flags) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<long long>(num_groups) * num_rotations) return;
  const int r = static_cast<int>(i / num_groups), g = static_cast<int>(i % num_groups);
  const int rx = r % side_r, ry = (r / side_r) % side_r, rz = r / (side_r * side_r);
  const int rb = ((rz >> 1) * blocks_per_axis + (ry >> 1)) * blocks_per_axis + (rx >> 1);
  const float threshold = __uint_as_float(*threshold_bits) * factor;
  if (computed[i] || !(block_upper[static_cast<size_t>(rb) * num_groups + g] >= threshold)) return;
  computed[i] = 1;
  flags[i] = 1;
}

// Rt3DSumBoundsKernel for a partly computed group table: pairs never computed get -1.
__global__ void Rt3DSumBoundsMaskedKernel(Rt3DBulkParams P, const uint8_t* __restrict__ computed) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const long long total = static_cast<long long>(P.num_rotations) * P.num_translations;
  float upper = 0.f;
  if (c < total) {
    if (computed[c]) {
      const int r = static_cast<int>(c / P.num_translations);
      const int t = static_cast<int>(c - static_cast<long long>(r) * P.num_translations);
      float lower;
      Bounds3D(P, P.sums[c].x, 0u, P.translation[t].w, r, &lower, &upper);
      P.upper[c] = upper;
    } else {
      P.upper[c] = -1.f;
    }
  }
  unsigned bits = __float_as_uint(upper);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits = max(bits, __shfl_xor(bits, off, 64));
  if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(P.max_upper_bits, bits);
}

// Debug switch rt3d_verify: every computed (rotation, group) bound against its block's.
__global__ void Rt3DVerifyBlocksKernel(const float* __restrict__ block_upper,
                                       const float* __restrict__ group_upper,
                                       const uint8_t* __restrict__ computed, int num_groups,
                                       int num_rotations, int side_r, int blocks_per_axis,
                                       int* __restrict__ violations) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<long long>(num_groups) * num_rotations || !computed[i]) return;
  const int r = static_cast<int>(i / num_groups), g = static_cast<int>(i % num_groups);
  const int rx = r % side_r, ry = (r / side_r) % side_r, rz = r / (side_r * side_r);
  const int rb = ((rz >> 1) * blocks_per_axis + (ry >> 1)) * blocks_per_axis + (rx >> 1);
  if (!(block_upper[static_cast<size_t>(rb) * num_groups + g] >= group_upper[i])) atomicAdd(violations, 1);
}

// Groups whose weighted upper bound reaches the threshold and that have not been expanded yet:
// their member translations are flagged for the next candidate pass.
//   threshold = *threshold_bits (as float) * factor.
__global__ void Rt3DSelectGroupsKernel(const float* __restrict__ group_upper, int num_groups,
                                       int num_rotations, int side, int groups_per_axis,
                                       const unsigned* __restrict__ threshold_bits, float factor,
                                       uint8_t* __restrict__ expanded,
                                       uint8_t* __restrict__ flags, int num_translations) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<long long>(num_groups) * num_rotations) return;
  const float threshold = __uint_as_float(*threshold_bits) * factor;
  if (expanded[i] || !(group_upper[i] >= threshold)) return;
  expanded[i] = 1;
  const int r = static_cast<int>(i / num_groups), g = static_cast<int>(i % num_groups);
  const int gx = g % groups_per_axis, gy = (g / groups_per_axis) % groups_per_axis,
            gz = g / (groups_per_axis * groups_per_axis);
  const int nx = min(2, side - 2 * gx), ny = min(2, side - 2 * gy), nz = min(2, side - 2 * gz);
  for (int c = 0; c < nz; ++c)
    for (int b = 0; b < ny; ++b)
      for (int a = 0; a < nx; ++a)
        flags[static_cast<size_t>(r) * num_translations +
              ((2 * gz + c) * side + (2 * gy + b)) * side + (2 * gx + a)] = 1;
}

// One block per work list (= `list_rotations` consecutive rotations): the flagged translations
// of its rotations, rotation by rotation in ascending order (x offsets fastest, so neighbouring
// lanes of the candidate pass read neighbouring cells), as entries w * T + t; flags cleared for
// the next round; one work descriptor (list, chunk) per `block_items` entries.
__global__ void __launch_bounds__(256)
Rt3DCompactKernel(uint8_t* __restrict__ flags, int num_translations, int num_rotations,
                  int list_rotations, int* __restrict__ counts, int* __restrict__ items,
                  int* __restrict__ total, int2* __restrict__ blocks,
                  int* __restrict__ num_blocks, int block_items) {
  __shared__ int wave_count[4];
  __shared__ int base;
  const int list = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* out = items + static_cast<size_t>(list) * list_rotations * num_translations;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int w = 0; w < list_rotations; ++w) {
    const int r = list * list_rotations + w;
    if (r >= num_rotations) break;
    uint8_t* f = flags + static_cast<size_t>(r) * num_translations;
    for (int t0 = 0; t0 < num_translations; t0 += 256) {
      const int t = t0 + tid;
      const bool on = t < num_translations && f[t] != 0;
      if (on) f[t] = 0;
      const unsigned long long mask = __ballot(on);
      if (lane == 0) wave_count[wave] = __popcll(mask);
      __syncthreads();
      int offset = base;
      for (int k = 0; k < wave; ++k) offset += wave_count[k];
      if (on) out[offset + __popcll(mask & ((1ull << lane) - 1ull))] = w * num_translations + t;
      __syncthreads();
      if (tid == 0) base += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
      __syncthreads();
    }
  }
  if (tid == 0) {
    counts[list] = base;
    if (base) {
      atomicAdd(total, base);
      const int chunks = (base + block_items - 1) / block_items;
      const int first = atomicAdd(num_blocks, chunks);
      for (int k = 0; k < chunks; ++k) blocks[first + k] = make_int2(list, k);
    }
  }
}

// Debug switch rt3d_crosscheck (tests): the tiled passes against the memory-gather kernels, element by
// element -- group upper bounds (bitwise) and candidate sums Q.
__global__ void Rt3DCompareFloatsKernel(const float* __restrict__ a, const float* __restrict__ b,
                                        long long n, int* __restrict__ mismatches) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n && __float_as_uint(a[i]) != __float_as_uint(b[i])) atomicAdd(mismatches, 1);
}
__global__ void Rt3DCompareSumsKernel(const uint2* __restrict__ a, const uint2* __restrict__ b,
                                      long long n, int* __restrict__ mismatches) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n && a[i].x != b[i].x) atomicAdd(mismatches, 1);
}

// out = the 3 x 3 x 3 dilation of the row-major brick `in`, through the scratch d_tmp.
void Dilate(Rt3DBoundsSearch* run, const uint8_t* in, uint8_t* out) {
  const Rt3DBulkGeometry& g = run->geo;
  const int bx = static_cast<int>(g.bx), by = static_cast<int>(g.by), bz = static_cast<int>(g.bz);
  DilateXKernel<<<DivUp(g.cells, 256), 256, 0, run->stream()>>>(in, run->d_tmp, bx, g.cells);
  DilateYZKernel<<<DivUp(g.cells, 256), 256, 0, run->stream()>>>(run->d_tmp, out, bx, by, bz);
}

// Row-major and tiled q bricks from the voxels or the resident brick, and the dilation.
void BuildBulkBricks(Rt3DBoundsSearch* run, const Rt3DGridSource& grid) {
  const Brick* resident = grid.resident;
  const int64_t num_voxels = grid.num_voxels;
  Workspace& ws = *run->ws;
  const Rt3DBulkGeometry& g = run->geo;
  const PaddedBrick& brick = run->D->brick;
  const int bx = static_cast<int>(g.bx), by = static_cast<int>(g.by);
  // [row-major q | tiled q]
  run->d_rows = ws.dev[kSlotQBrick].ReserveAs<uint8_t>(g.cells + 128 + g.tiled_cells);
  run->d_tiled = run->d_rows + (g.cells + 127) / 128 * 128;
  run->d_dilated = ws.dev[kSlotDilated].ReserveAs<uint8_t>(g.cells);
  run->d_tmp = ws.dev[kSlotScratch].ReserveAs<uint8_t>(
      std::max<size_t>(g.cells, sizeof(uint2) * static_cast<size_t>(run->S->num_candidates)));
  CMX_HIP(hipMemsetAsync(run->d_rows, 0, (run->d_tiled - run->d_rows) + g.tiled_cells, ws.stream));
  if (resident != nullptr) {
    const long long count = static_cast<long long>(resident->nx) * resident->ny * resident->nz;
    BrickBulkKernel<<<DivUp(count, 256), 256, 0, ws.stream>>>(
        static_cast<const uint16_t*>(resident->cells), count, resident->nx, resident->ny, g.pad,
        bx, by, g.tiles_y, g.pitch_z, run->d_rows, run->d_tiled);
  } else if (num_voxels > 0) {
    ScatterBulkKernel<<<DivUp(num_voxels, 256), 256, 0, ws.stream>>>(
        run->D->d_vox, num_voxels, brick.lo_x, brick.lo_y, brick.lo_z, g.pad, bx, by, g.tiles_y,
        g.pitch_z, run->d_rows, run->d_tiled);
  }
  Dilate(run, run->d_rows, run->d_dilated);
}

// Group table, bound arrays, flags and the misc block; everything a call starts from zeroed.
void ReserveBoundsBuffers(Rt3DBoundsSearch* run) {
  Workspace& ws = *run->ws;
  const Rt3DSearchSpace& S = *run->S;
  const long long RG = run->RG;
  run->d_group = ws.dev[kSlotGroups].ReserveAs<float4>(S.G);
  run->d_group_upper = ws.dev[kSlotGroupUpper].ReserveAs<float>(RG);
  run->d_expanded = ws.dev[kSlotFlags].ReserveAs<uint8_t>(RG + S.num_candidates);
  run->d_flags = run->d_expanded + RG;
  run->d_upper = run->D->d_weighted;
  run->d_items = reinterpret_cast<int*>(run->D->d_unweighted);
  // work descriptors of a round: at most one per 256 translations and rotation
  const int max_blocks = static_cast<int>(S.R) * DivUp(S.T, kCand3DThreads);   // (>= any block size used)
  const size_t counts_bytes = (sizeof(int) * S.R + 15) / 16 * 16;
  char* d_bmisc = static_cast<char*>(ws.dev[kSlotBulkMisc].Reserve(
      sizeof(Rt3DBulkHead) + counts_bytes + sizeof(int2) * max_blocks + sizeof(Rt3DCounters)));
  run->d_head = reinterpret_cast<Rt3DBulkHead*>(d_bmisc);
  run->d_counts = reinterpret_cast<int*>(run->d_head + 1);
  run->d_blocks = reinterpret_cast<int2*>(d_bmisc + sizeof(Rt3DBulkHead) + counts_bytes);
  run->d_counters = reinterpret_cast<Rt3DCounters*>(run->d_blocks + max_blocks);
  run->h_read = &run->D->pinned->bounds;
  run->h_head = static_cast<Rt3DBulkHead*>(ws.pinned[kPinnedBulkHead].Reserve(sizeof(Rt3DBulkHead)));
  float4* h_group = ws.pinned[kPinnedGroups].ReserveAs<float4>(S.G);
  std::memcpy(h_group, S.group.data(), sizeof(float4) * S.G);
  CMX_HIP(hipMemcpyAsync(run->d_group, h_group, sizeof(float4) * S.G, hipMemcpyHostToDevice,
                         ws.stream));
  CMX_HIP(hipMemsetAsync(run->d_head, 0, kBulkHeadZeroed, ws.stream));
  CMX_HIP(hipMemsetAsync(run->d_counters, 0, sizeof(Rt3DCounters), ws.stream));
  CMX_HIP(hipMemsetAsync(run->d_counts, 0, sizeof(int) * S.R, ws.stream));
  CMX_HIP(hipMemsetAsync(run->d_expanded, 0, RG + S.num_candidates, ws.stream));
  CMX_HIP(hipMemsetAsync(run->d_upper, 0, sizeof(float) * S.num_candidates, ws.stream));
}

// What every bulk pass shares: index arithmetic, clamp range, bound constants.
Rt3DBulkParams BaseBulkParams(const Rt3DBoundsSearch& run) {
  const Rt3DSearchSpace& S = *run.S;
  const Rt3DBulkGeometry& g = run.geo;
  const PaddedBrick& brick = run.D->brick;
  const int n = S.n, pad = g.pad, reach = g.reach;
  const float resolution = S.resolution;
  Rt3DBulkParams B{};
  B.cell_count = static_cast<unsigned>(g.cells);
  B.pitch_x = static_cast<float>(g.bx); B.pitch_y = static_cast<float>(g.by);
  B.off_x = static_cast<float>(pad - brick.lo_x);
  B.off_y = static_cast<float>(pad - brick.lo_y);
  B.off_z = static_cast<float>(pad - brick.lo_z);
  B.inv_resolution = 1.f / resolution;
  double q_abs = 0.;
  const int los[3] = {brick.lo_x, brick.lo_y, brick.lo_z};
  const int dims[3] = {brick.nx, brick.ny, brick.nz};
  for (int k = 0; k < 3; ++k)
    q_abs = std::max<double>(q_abs, std::max(std::abs(los[k] - pad),
                                             std::abs(los[k] + dims[k] - 1 + pad)));
  const double q_pad = static_cast<double>(std::max(g.bx, std::max(g.by, g.bz)));
  // |q - (qe + off)| <= (2 |c / res| + |q|) 2^-24 (rounded 1/res, one fma rounding, the
  // reference's rounded quotient qe); 25 % on top.
  const double e = (2. * q_abs + q_pad + 4.) * 0x1p-24 * 1.25;
  B.guard = std::nextafter(static_cast<float>(0.5 - e), 0.f);
  B.t0x = S.init.t.x; B.t0y = S.init.t.y; B.t0z = S.init.t.z;
  B.lo_x = (brick.lo_x - reach - 1) * resolution;
  B.hi_x = (brick.lo_x + brick.nx + reach) * resolution;
  B.lo_y = (brick.lo_y - reach - 1) * resolution;
  B.hi_y = (brick.lo_y + brick.ny + reach) * resolution;
  B.lo_z = (brick.lo_z - reach - 1) * resolution;
  B.hi_z = (brick.lo_z + brick.nz + reach) * resolution;
  B.num_rotations = static_cast<int>(S.R);
  B.n = n;
  B.rotation = run.D->d_rot; B.rotation_angle = run.D->d_angle;
  B.wt = run.D->P.wt; B.wr = run.D->P.wr;
  const float kMinP = 0.1f, kMaxP = 1.f - kMinP;
  const float scale = (kMaxP - kMinP) / (32768 - 2.f);
  B.min_probability = kMinP;
  B.scale_over_n = 128. * static_cast<double>(scale) / n;
  B.slack_hi = 127. * static_cast<double>(scale) + 2e-7;
  const double ku = (n + 8.) * 0x1p-24;
  B.delta = ku / (1. - ku) * 1.01 + 2e-6;
  B.max_lower_bits = &run.d_head->max_lower; B.max_upper_bits = &run.d_head->max_upper;
  return B;
}

// ---- the stages -------------------------------------------------------------------------------

// Compacts flags[R][width] into the work lists, `block_items` entries per work block, and adds
// their number to *d_total; returns the work blocks of the lists -- what the next launch is
// sized by: one sync per list (tens of microseconds) instead of hundreds of thousands of blocks
// that find nothing to do.  with_segments: the chunk counts come back in the same sync.
int CompactAndReadBack(Rt3DBoundsSearch* run, uint8_t* d_flags, int width, int* d_total,
                       int block_items, bool with_segments) {
  Workspace& ws = *run->ws;
  Rt3DCompactKernel<<<run->num_lists, 256, 0, ws.stream>>>(
      d_flags, width, static_cast<int>(run->S->R), run->mode.list_rotations, run->d_counts,
      run->d_items, d_total, run->d_blocks, &run->d_counters->num_blocks, block_items);
  CMX_HIP(hipMemcpyAsync(&run->h_read->num_blocks, &run->d_counters->num_blocks, sizeof(int),
                         hipMemcpyDeviceToHost, ws.stream));
  if (with_segments)
    CMX_HIP(hipMemcpyAsync(run->h_read->segments, run->d_segment_counts,
                           sizeof(int) * kNumSegmentCounts, hipMemcpyDeviceToHost, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));
  return run->h_read->num_blocks;
}

int ReadBackInt(Workspace& ws, const int* d_value) {
  int value = -1;
  CMX_HIP(hipMemcpyAsync(&value, d_value, sizeof(int), hipMemcpyDeviceToHost, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));
  return value;
}

// Blocks of 2 x 2 x 2 rotations x groups: the group pass over the centre rotations and the
// twice-dilated brick.
void RotationBlockPass(Rt3DBoundsSearch* run) {
  Workspace& ws = *run->ws;
  run->d_dilated_twice = ws.dev[kSlotDilatedTwice].ReserveAs<uint8_t>(run->geo.cells);
  Dilate(run, run->d_dilated, run->d_dilated_twice);
  // [sums | bounds | the best bound's bits]
  const long long RbG = run->S->Rb * run->S->G;
  const size_t bounds_bytes = (sizeof(uint2) + sizeof(float)) * RbG + 16;
  char* d_block = static_cast<char*>(ws.dev[kSlotBlockBounds].Reserve(bounds_bytes));
  run->d_block_sums = reinterpret_cast<uint2*>(d_block);
  run->d_block_upper = reinterpret_cast<float*>(d_block + sizeof(uint2) * RbG);
  run->d_block_max = reinterpret_cast<unsigned*>(run->d_block_upper + RbG);
  CMX_HIP(hipMemsetAsync(d_block, 0, bounds_bytes, ws.stream));
  run->d_computed = ws.dev[kSlotPairs].ReserveAs<uint8_t>(2 * run->RG);
  CMX_HIP(hipMemsetAsync(run->d_computed, 0, 2 * run->RG, ws.stream));
  TileGroups(run, /*rotation_blocks=*/true);
  Rt3DSumBoundsKernel<<<DivUp(RbG, 256), 256, 0, ws.stream>>>(BlockParams(*run));
  run->trace->Mark("rotation blocks");
}

// One round of the sparse group pass: the pairs of the rotation blocks `factor` * the threshold
// cannot exclude and that no earlier round has computed.
void PairRound(Rt3DBoundsSearch* run, const unsigned* threshold_bits, float factor) {
  Workspace& ws = *run->ws;
  const Rt3DSearchSpace& S = *run->S;
  const long long RG = run->RG;
  const int G = S.G, R = static_cast<int>(S.R);
  uint8_t* d_pair_flags = run->d_computed + RG;
  CMX_HIP(hipMemsetAsync(&run->d_counters->num_blocks, 0, sizeof(int), ws.stream));
  Rt3DSelectPairsKernel<<<DivUp(RG, 256), 256, 0, ws.stream>>>(
      run->d_block_upper, G, R, S.side_r, S.Ab, threshold_bits, factor, run->d_computed,
      d_pair_flags);
  const int nbq = CompactAndReadBack(run, d_pair_flags, G, &run->d_counters->pair_total,
                                     kPairItems, /*with_segments=*/true);
  const int list_chunks = run->h_read->segments[kCandidateChunks];
  if (nbq > 0 && list_chunks > 0) TilePairs(run, nbq, list_chunks);
  Rt3DSumBoundsMaskedKernel<<<DivUp(RG, 256), 256, 0, ws.stream>>>(GroupParams(*run),
                                                                   run->d_computed);
  if (run->mode.verify)
    Rt3DVerifyBlocksKernel<<<DivUp(RG, 256), 256, 0, ws.stream>>>(
        run->d_block_upper, run->d_group_upper, run->d_computed, G, R, S.side_r, S.Ab,
        &run->d_counters->violations);
}

// The group pass on the memory gathers.  Flat (rotation, group) lanes: as many whole wavefronts
// per block as fit G + 1 lanes.
void GatherGroupPass(Rt3DBoundsSearch* run, const Rt3DBulkParams& P) {
  const int G = run->S->G;
  const long long R = run->S->R;
  const int flat_threads = std::min(kBulk3DThreads, (G + 1) / 64 * 64);
  if (flat_threads >= 128 && R >= 2)
    Rt3DBulkKernel<true><<<DivUp(run->RG, flat_threads), flat_threads, 0, run->stream()>>>(
        P, run->D->d_xyz);
  else
    Rt3DBulkKernel<true><<<dim3(DivUp(G, kBulk3DThreads), std::max<unsigned>(2u, R)),
                           kBulk3DThreads, 0, run->stream()>>>(P, run->D->d_xyz);
}

// rt3d_crosscheck: the gather kernel's group bounds next to the tiled ones, compared bitwise.
void CrossCheckGroupPass(Rt3DBoundsSearch* run) {
  Workspace& ws = *run->ws;
  const long long RG = run->RG;
  Rt3DBulkParams B2 = GroupParams(*run);
  float* d_upper2 = ws.dev[kSlotCrosscheck].ReserveAs<float>(RG + 4);
  B2.upper = d_upper2;
  B2.max_upper_bits = reinterpret_cast<unsigned*>(d_upper2 + RG);
  int* d_mismatch = reinterpret_cast<int*>(d_upper2 + RG + 1);
  CMX_HIP(hipMemsetAsync(d_upper2 + RG, 0, 16, ws.stream));
  GatherGroupPass(run, B2);
  Rt3DCompareFloatsKernel<<<DivUp(RG, 256), 256, 0, ws.stream>>>(run->d_group_upper, d_upper2, RG,
                                                                 d_mismatch);
  const int mismatches = ReadBackInt(ws, d_mismatch);
  CMX_REQUIRE(mismatches == 0,
              "internal error: %d of %lld tiled group bounds differ from the gather kernel's",
              mismatches, RG);
}

// The group level between ev_k0 and ev_k1: upper bounds of (rotation, group) pairs.
void GroupLevel(Rt3DBoundsSearch* run) {
  if (!run->mode.use_tiles) {
    GatherGroupPass(run, GroupParams(*run));
    return;
  }
  Workspace& ws = *run->ws;
  const size_t sums_bytes = sizeof(uint2) * run->RG * (run->mode.staged ? 2 : 1);
  run->d_group_sums = reinterpret_cast<uint2*>(ws.dev[kSlotGroupSums].Reserve(sums_bytes));
  CMX_HIP(hipMemsetAsync(run->d_group_sums, 0, sums_bytes, ws.stream));
  BoxListChunks(run);
  if (run->mode.rotblocks) {
    RotationBlockPass(run);
    // first round: the pairs of the blocks next to the best block bound
    PairRound(run, run->d_block_max, run->mode.first_pair_factor);
  } else {
    TileGroups(run, /*rotation_blocks=*/false);
    Rt3DSumBoundsKernel<<<DivUp(run->RG, 256), 256, 0, ws.stream>>>(GroupParams(*run));
  }
  if (run->tiles.stats) ReportGroupTiles(run);
  if (run->mode.crosscheck) CrossCheckGroupPass(run);
}

// Flags the members of the groups `round`'s threshold cannot exclude and compacts them into
// work lists; returns the number of work blocks.  (The staged second round sizes its launches by
// the chunk counts round 0 reads back.)
int SelectCandidates(Rt3DBoundsSearch* run, int round) {
  const Rt3DSearchSpace& S = *run->S;
  const int R = static_cast<int>(S.R), T = static_cast<int>(S.T);
  Rt3DSelectGroupsKernel<<<DivUp(run->RG, 256), 256, 0, run->stream()>>>(
      run->d_group_upper, S.G, R, S.side_t, S.gpa,
      round == 0 ? &run->d_head->max_upper : &run->d_head->max_lower,
      round == 0 ? run->mode.first_round_factor : 1.f, run->d_expanded, run->d_flags, T);
  return run->round_blocks[round] =
             CompactAndReadBack(run, run->d_flags, T, &run->d_head->total, run->mode.block_items,
                                /*with_segments=*/run->mode.staged && round == 0);
}

// rt3d_crosscheck: the same work lists on the gather kernel, into a second (Q, A) array.
void CrossCheckCandidateRound(Rt3DBoundsSearch* run, const Rt3DBulkParams& BC, int round, int nb) {
  Workspace& ws = *run->ws;
  const long long num_candidates = run->S->num_candidates;
  const size_t bytes = sizeof(uint2) * static_cast<size_t>(num_candidates) + 16;
  Rt3DBulkParams B2 = BC;
  uint2* d_sums2 = reinterpret_cast<uint2*>(ws.dev[kSlotCrosscheck].Reserve(bytes));
  int* d_mismatch = reinterpret_cast<int*>(d_sums2 + num_candidates);
  B2.sums = d_sums2;
  B2.cells = run->d_tiled;
  B2.cell_count = static_cast<unsigned>(run->geo.tiled_cells);
  if (round == 0) CMX_HIP(hipMemsetAsync(d_sums2, 0, bytes, ws.stream));
  B2.slice_points = DivUp(run->S->n, kBulk3DChunk) * kBulk3DChunk;
  Rt3DBulkKernel<false><<<dim3(nb, 1, 1), run->mode.block_items, 0, ws.stream>>>(B2, run->D->d_xyz);
  Rt3DCompareSumsKernel<<<DivUp(num_candidates, 256), 256, 0, ws.stream>>>(
      BC.sums, d_sums2, num_candidates, d_mismatch);
  const int mismatches = ReadBackInt(ws, d_mismatch);
  CMX_REQUIRE(mismatches == 0,
              "internal error: %d tiled candidate sums differ from the gather kernel's",
              mismatches);
}

// One candidate round in one piece: the (Q, A) sums of `nb` work blocks, then their bounds.
void CandidateRound(Rt3DBoundsSearch* run, int round, int nb) {
  Workspace& ws = *run->ws;
  const int n = run->S->n, block_items = run->mode.block_items;
  Rt3DBulkParams BC = CandidateParams(*run);
  if (run->mode.use_tiles) {
    TileCandidates(run, nb, 0, 2, run->max_chunks);
    if (run->mode.crosscheck) CrossCheckCandidateRound(run, BC, round, nb);
  } else {
    // Points are split over blockIdx.z until the launch is ~32 blocks per CU.
    // (blocks of two wavefronts: sixteen fit a CU)
    const int want = std::max(1, DivUp(32 * run->cus, nb));
    BC.slice_points = std::max(1, DivUp(DivUp(n, want), kBulk3DChunk)) * kBulk3DChunk;
    const dim3 cand_grid(nb, 1, DivUp(n, BC.slice_points));
    Rt3DBulkKernel<false><<<cand_grid, kCand3DThreads, 0, ws.stream>>>(BC, run->D->d_xyz);
  }
  Rt3DBoundsKernel<<<nb, block_items, 0, ws.stream>>>(BC);
  if (run->mode.verify)
    Rt3DVerifyKernel<<<nb, block_items, 0, ws.stream>>>(
        BC, run->d_group_upper, run->S->G, run->S->side_t, run->S->gpa,
        &run->d_counters->violations);
  run->trace->Mark(round == 0 ? "candidate pass 1" : "candidate pass 2");
}

// The second candidate round segment by segment; after the first and the second, the
// candidates whose bound (own sum so far + the group's sum over the rest) has fallen below the
// best lower bound leave the work lists.  Verification mode keeps the lists and records the
// decisions instead (Rt3DStageCheckKernel).
void StagedSecondRound(Rt3DBoundsSearch* run, int nb) {
  Workspace& ws = *run->ws;
  const Rt3DSearchSpace& S = *run->S;
  const bool verify = run->mode.verify;
  const int block_items = run->mode.block_items;
  const Rt3DBulkParams BC = CandidateParams(*run);
  unsigned long long* d_stage_ub = nullptr;
  uint8_t* d_dropped = nullptr;
  if (verify) {
    d_stage_ub = ws.dev[kSlotStageBounds].ReserveAs<unsigned long long>(
        static_cast<size_t>(S.num_candidates));
    d_dropped = ws.dev[kSlotStageDropped].ReserveAs<uint8_t>(static_cast<size_t>(S.num_candidates));
  }
  const int* seg = run->h_read->segments;
  const int seg_chunks[3] = {seg[kCandidateSegments],
                             seg[kCandidateSegments + 1] - seg[kCandidateSegments],
                             seg[kCandidateChunks] - seg[kCandidateSegments + 1]};
  int live = nb;
  for (int stage = 0; stage < 3 && live > 0; ++stage) {
    if (seg_chunks[stage] > 0) TileCandidates(run, live, stage, stage, seg_chunks[stage]);
    if (stage == 2) break;
    Rt3DStageFilterKernel<<<live, block_items, 0, ws.stream>>>(
        BC, run->d_group_sums, run->d_group_sums + run->RG, S.G, S.side_t, S.gpa, stage,
        run->d_flags, d_stage_ub, d_dropped);
    if (verify) continue;
    CMX_HIP(hipMemsetAsync(&run->d_counters->num_blocks, 0, sizeof(int), ws.stream));
    live = CompactAndReadBack(run, run->d_flags, static_cast<int>(S.T),
                              &run->d_counters->stage_total, block_items, /*with_segments=*/false);
    run->stage_blocks[stage] = live;
  }
  if (live > 0) {
    Rt3DBoundsKernel<<<live, block_items, 0, ws.stream>>>(BC);
    if (verify) {
      Rt3DStageCheckKernel<<<live, block_items, 0, ws.stream>>>(BC, d_stage_ub, d_dropped,
                                                                &run->d_counters->violations);
      Rt3DVerifyKernel<<<live, block_items, 0, ws.stream>>>(
          BC, run->d_group_upper, S.G, S.side_t, S.gpa, &run->d_counters->violations);
    }
  }
  run->trace->Mark("candidate pass 2 (staged)");
}

// Everything within 1e-5 of the best lower bound, scored exactly; false: a flat score landscape
// (more finalists than the list holds) -- every candidate on the per-candidate kernel then.
bool CollectFinalists(Rt3DBoundsSearch* run, Rt3DFinalists* out) {
  Workspace& ws = *run->ws;
  const Rt3DSearchSpace& S = *run->S;
  CollectAndScoreFinalists(run);
  run->trace->Mark("finalists");
  CMX_HIP(hipGetLastError());
  RecordEvent(ws.ev_end, ws.stream);
  CMX_HIP(hipMemcpyAsync(run->h_head, run->d_head, sizeof(Rt3DBulkHead), hipMemcpyDeviceToHost,
                         ws.stream));
  CMX_HIP(hipMemcpyAsync(&run->h_read->pair_total, &run->d_counters->pair_total, sizeof(int),
                         hipMemcpyDeviceToHost, ws.stream));
  CMX_HIP(hipStreamSynchronize(ws.stream));
  run->trace->Report();
  const Rt3DBulkHead& head = *run->h_head;
  if (run->mode.verify) {
    int violations = 0;
    CMX_HIP(hipMemcpy(&violations, &run->d_counters->violations, sizeof(int),
                      hipMemcpyDeviceToHost));
    CMX_REQUIRE(violations == 0,
                "internal error: %d bound violations (a group bound below a member's lower "
                "bound, or a staged bound below the candidate's final sum)", violations);
  }
  // rotation blocks: their bounds + the pairs that went through the group pass
  const long long group_bounds =
      run->mode.rotblocks ? S.Rb * S.G + run->h_read->pair_total : run->RG;
  if (run->mode.report) {
    float lo_f, up_f;
    std::memcpy(&lo_f, &head.max_lower, 4);
    std::memcpy(&up_f, &head.max_upper, 4);
    fprintf(stderr,
            "[cmx] rt3d: group pass %.3f ms (%lld bounds), %d of %lld candidates scored, "
            "%d finalists, best lower %.6f, best group upper %.6f, work blocks %d + %d "
            "(staged: %d after a quarter of the points, %d after half), device %.3f ms\n",
            ElapsedMs(ws.ev_k0, ws.ev_k1), group_bounds, head.total, S.num_candidates, head.count,
            lo_f, up_f, run->round_blocks[0], run->round_blocks[1], run->stage_blocks[0],
            run->stage_blocks[1], ElapsedMs(ws.ev_begin, ws.ev_end));
  }
  if (head.count < 1 || head.count > kBulkFinalistCap) return false;
  std::vector<std::pair<long long, float>> pairs(head.count);
  for (int i = 0; i < head.count; ++i) {
    const long long r = head.finalists[i] / S.T, t = head.finalists[i] % S.T;
    pairs[i] = {t * S.R + r, head.exact[i]};
  }
  std::sort(pairs.begin(), pairs.end());
  out->index.resize(head.count);
  out->acc.resize(head.count);
  for (int i = 0; i < head.count; ++i) {
    out->index[i] = pairs[i].first;
    out->acc[i] = pairs[i].second;
  }
  out->num_finalists = head.count;
  out->group_bounds = group_bounds;
  out->bounds_evaluated = group_bounds + head.total;
  return true;
}

}  // namespace

// The bounds search; false when it did not narrow the search down (see CollectFinalists).
bool RunBoundsSearch(Workspace& ws, const Rt3DSearchSpace& S, const Rt3DMode& mode,
                     const Rt3DBulkGeometry& geo, const Rt3DDevice& D, const Rt3DGridSource& grid,
                     Rt3DFinalists* out) {
  Rt3DBoundsSearch run;
  run.ws = &ws; run.S = &S; run.D = &D; run.mode = mode; run.geo = geo;
  run.RG = S.R * S.G;
  run.num_lists = DivUp(S.R, mode.list_rotations);
  BuildBulkBricks(&run, grid);
  ReserveBoundsBuffers(&run);
  run.base = BaseBulkParams(run);
  run.trace.emplace(ws.stream);
  run.trace->Mark("bricks");
  (void)hipDeviceGetAttribute(&run.cus, hipDeviceAttributeMultiprocessorCount, ws.device);
  if (mode.use_tiles) SortCloudIntoBins(&run);
  RecordEvent(ws.ev_k0, ws.stream);
  GroupLevel(&run);
  RecordEvent(ws.ev_k1, ws.stream);
  // Candidate pass, twice: the members of the groups next to the best upper bound yield a
  // lower bound; then everything that lower bound cannot exclude.  (The threshold only
  // rises afterwards, so no third round can add a group.)
  CMX_HIP(hipMemsetAsync(run.d_tmp, 0, sizeof(uint2) * static_cast<size_t>(S.num_candidates),
                         ws.stream));
  run.trace->Mark("group pass");
  for (int round = 0; round < 2; ++round) {
    CMX_HIP(hipMemsetAsync(&run.d_counters->num_blocks, 0, sizeof(int), ws.stream));
    if (round == 1 && mode.rotblocks) {
      // the pairs of every rotation block the lower bound of round 0 cannot exclude
      RecordEvent(ws.ev_x0, ws.stream);
      PairRound(&run, &run.d_head->max_lower, 1.f);
      RecordEvent(ws.ev_x1, ws.stream);
      out->second_pairs_pass = true;
      CMX_HIP(hipMemsetAsync(&run.d_counters->num_blocks, 0, sizeof(int), ws.stream));
      run.trace->Mark("group pass 2 (pairs)");
    }
    const int nb = SelectCandidates(&run, round);
    if (nb == 0) continue;
    if (mode.staged && round == 1) {
      StagedSecondRound(&run, nb);
    } else {
      CandidateRound(&run, round, nb);
    }
  }
  return CollectFinalists(&run, out);
}

}  // namespace cmx
