// What the TSDF sources (fusion.hip, tsdf_mesh.hip) share: the grid of a volume, the size and parameter checks of the entry points and
// the rule that makes a voxel valid for the surface extraction.
#pragma once

struct TsdfGrid {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
};

static inline bool tsdf_dims_ok(int nx, int ny, int nz) {
    return nx > 0 && ny > 0 && nz > 0 && (long)nx * ny < (1L << 31) && (long)nx * ny * nz < (1L << 31);
}

static inline bool tsdf_positive(float v) { return v > 0.f; }                 // false for NaN

// a voxel takes part in the surface: enough weight and a value strictly inside the truncation band (false for NaN)
__device__ __forceinline__ bool tsdf_valid(float t, float w, float min_weight) { return w >= min_weight && fabsf(t) < 1.f; }
