// World point cloud for gfx950 (include/ikflow_amd_cloud.h): the clearance of every row's configuration from the handle's cloud, by brute force -
// no acceleration structure, nothing that can go stale or out of range.
//
// k_cloud_clearance: grid (row tiles x chunks), 256 threads, a tile of 64 rows; lane t & 63 owns a row, wave t >> 6 a quarter (128 points) of
// every 512-point tile of the workgroup's chunk.  Phase 1: wave 0 walks the chain once per row and leaves the row's capsule end points in LDS
// (one slice per lane, stride (6 n_caps) | 1: odd, so the lanes' slices start in different banks).  Phase 2, per tile: the 256 threads stage
// the tile (one 16-byte global load per thread and pass, 8192 B); then every wave loops over the capsules - axis to registers once - and over its
// 128 points, every lane reading the same float4 (one LDS broadcast per point-capsule term, no global load), and folds sqrtf(min2) - rc of the
// (capsule, tile) into ONE register: exact, because sqrtf and x - rc are monotone (cloud_math.h), and no per-capsule array indexed at run time
// that would go to scratch.  After the last tile the four waves' values of a row meet through 64 x 4 words of LDS; wave 0 takes r off and writes
// the call's outputs (one chunk) or partial[chunk][row] (more), which k_cloud_merge - a thread per row - reduces.  No atomics, no waiting between
// workgroups, no inline assembly, no scratch.  Rows beyond n in the last row tile do no work and store nothing; a call of fewer than 64 rows
// leaves lanes idle (the candidate stage never has so few rows that it matters).
// Dynamic LDS: 8192 B tile (first: the float4 reads need the 16-byte aligned base) + 1024 B hand-over + 64 x ((6 n_caps) | 1) floats.
#include "ikf_internal.h"

namespace ikf {

constexpr size_t kCloudMaxLds = sizeof(float4) * IKF_CLOUD_TILE + sizeof(float) * IKF_CLOUD_BLOCK + sizeof(float) * IKF_CLOUD_ROWS * (IKF_MAX_CAPSULES * 6 + 1);
static_assert(kCloudMaxLds == 8192 + 1024 + 37120, "point tile + hand-over + capsule slices");
static_assert(kCloudMaxLds <= 48 * 1024, "k_cloud_clearance takes no dynamic-LDS opt-in");
static_assert(IKF_CLOUD_BLOCK == 4 * IKF_CLOUD_ROWS && IKF_CLOUD_TILE == 2 * IKF_CLOUD_BLOCK, "four waves of 64 rows; two staging passes per tile");

template <int NDOF>
__global__ __launch_bounds__(IKF_CLOUD_BLOCK) void k_cloud_clearance(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, int cap_stride,
                                                                     const float4* __restrict__ pts, int tiles, int tiles_per_chunk, float point_radius,
                                                                     float min_clearance, const float* __restrict__ q, long long n,
                                                                     float* __restrict__ clearance, uint8_t* __restrict__ colliding,
                                                                     float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float4 cloud_lds[];
  float4* const PT = cloud_lds;                                                    // [512] the staged tile
  float* const HAND = reinterpret_cast<float*>(cloud_lds + IKF_CLOUD_TILE);      // [4][64] the waves' values of a row
  float* const W = HAND + IKF_CLOUD_BLOCK;                                         // [64][cap_stride] capsule end points
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long row = (long long)blockIdx.x * IKF_CLOUD_ROWS + lane;
  const bool live = row < n;
  const int nc = cm->n_caps;
  const float* const w = W + lane * cap_stride;
  if (wave == 0 && live) {
    float qv[NDOF];
    load_q<NDOF>(q, row, qv);
    capsule_endpoints<NDOF>(ch, cm, qv, W + lane * cap_stride);
  }
  const int tile_begin = blockIdx.y * tiles_per_chunk;
  const int tile_end = tile_begin + tiles_per_chunk < tiles ? tile_begin + tiles_per_chunk : tiles;
  float best = IKF_CLOUD_EMPTY;
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    __syncthreads();   // the end points are written (first tile); every wave has read the previous tile (later ones)
    const float4* const src = pts + (long long)tile * IKF_CLOUD_TILE;
    PT[t] = src[t];
    PT[t + IKF_CLOUD_BLOCK] = src[t + IKF_CLOUD_BLOCK];
    __syncthreads();
    if (!live) continue;   // (lanes of a dead row are dead in every wave; the barriers above are outside this branch)
    const float4* const mine = PT + wave * (IKF_CLOUD_TILE / 4);
    for (int c = 0; c < nc; ++c) {
      const CloudAxis ax = cloud_axis(w + c * 6, w + c * 6 + 3);
      const float rc = cm->radius[c];   // (the same address in every lane: a scalar load)
      float m2 = IKF_CLOUD_EMPTY;
#pragma unroll 8
      for (int i = 0; i < IKF_CLOUD_TILE / 4; ++i) {
        const float4 p = mine[i];
        m2 = fminf(m2, point_segment_dist2(p.x, p.y, p.z, ax));
      }
      best = fminf(best, sqrtf(m2) - rc);
    }
  }
  HAND[wave * IKF_CLOUD_ROWS + lane] = best;
  __syncthreads();
  if (wave != 0 || !live) return;
  best = fminf(fminf(HAND[lane], HAND[IKF_CLOUD_ROWS + lane]), fminf(HAND[2 * IKF_CLOUD_ROWS + lane], HAND[3 * IKF_CLOUD_ROWS + lane]));
  best = nc > 0 ? best - point_radius : IKF_CLOUD_EMPTY;
  if (gridDim.y > 1) {
    partial[(long long)blockIdx.y * n + row] = best;
    return;
  }
  if (clearance) clearance[row] = best;
  if (colliding) colliding[row] = best < min_clearance ? 1 : 0;
}

// The chunks' values of a row, reduced by one thread; writes the call's outputs.  chunks == 0: an empty cloud, 3.0e38 / 0 on every row.
__global__ __launch_bounds__(256) void k_cloud_merge(const float* __restrict__ partial, int chunks, float min_clearance, long long n,
                                                     float* __restrict__ clearance, uint8_t* __restrict__ colliding) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float best = IKF_CLOUD_EMPTY;
  for (int c = 0; c < chunks; ++c) best = fminf(best, partial[(long long)c * n + row]);
  if (clearance) clearance[row] = best;
  if (colliding) colliding[row] = chunks > 0 && best < min_clearance ? 1 : 0;
}

hipError_t launch_cloud_clearance(const Chain* ch, const CollisionModel* cm, int n_caps, const CloudPoint* pts, long long n_points,
                                  float point_radius, float min_clearance, int ndof, const float* q, long long n, int n_cu, float* clearance,
                                  uint8_t* colliding, float* partial, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!ch || !cm || !q || n_caps < 0 || n_caps > IKF_MAX_CAPSULES || n_points < 0 || n_points > IKF_CLOUD_MAX_POINTS || (n_points > 0 && !pts))
    return hipErrorInvalidValue;
  const unsigned merge_blocks = (unsigned)((n + 255) / 256);
  if (n_points == 0) {
    if (clearance || colliding) hipLaunchKernelGGL(k_cloud_merge, dim3(merge_blocks), dim3(256), 0, s, nullptr, 0, min_clearance, n, clearance, colliding);
    return hipGetLastError();
  }
  const CloudPlan plan = cloud_plan(n, n_points, n_cu);
  const int tiles = (int)cloud_tiles(n_points);
  if (plan.chunks < 1 || plan.chunks > IKF_CLOUD_MAX_CHUNKS || (long long)plan.chunks * plan.tiles_per_chunk < tiles ||
      (long long)(plan.chunks - 1) * plan.tiles_per_chunk >= tiles || (plan.chunks > 1 && !partial))
    return hipErrorInvalidValue;
  const int cap_stride = (n_caps * 6) | 1;
  const size_t lds = sizeof(float4) * IKF_CLOUD_TILE + sizeof(float) * (IKF_CLOUD_BLOCK + IKF_CLOUD_ROWS * (size_t)cap_stride);
  const dim3 grid((unsigned)((n + IKF_CLOUD_ROWS - 1) / IKF_CLOUD_ROWS), (unsigned)plan.chunks);
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_cloud_clearance<ND>), grid, dim3(IKF_CLOUD_BLOCK), lds, s, ch, cm, cap_stride,
                                             reinterpret_cast<const float4*>(pts), tiles, plan.tiles_per_chunk, point_radius, min_clearance, q, n,
                                             clearance, colliding, partial));
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (plan.chunks > 1 && (clearance || colliding))
    hipLaunchKernelGGL(k_cloud_merge, dim3(merge_blocks), dim3(256), 0, s, partial, plan.chunks, min_clearance, n, clearance, colliding);
  return hipGetLastError();
}

}  // namespace ikf
