// The triangle mesh of a truncated signed distance volume: marching tetrahedra on the Kuhn split of every cell.   gfx950 / wave64
//
// One thread per voxel, 256 consecutive voxels (x fastest) per workgroup, the volume caller-owned and read only; nothing survives a
// call and there are no atomics.  The definition is written out in include/unimatch_hip.h (um_tsdf_mesh); five launches:
//
//   cells      code[p], 16 bits per voxel: bit m (0..7) = corner p + m of cell p is inside (t < 0), bit 8 = the cell is active (p is a
//              cell and all eight corners are valid).  The only pass that reads the eight (tsdf, weight) taps of a cell.
//   classify   mask[p], 8 bits per voxel: bit e - 1 = the owned edge (p, e) carries a vertex, from the codes of the up to seven cells
//              p - s that contain an edge of p (all active cells of an edge agree on its two signs); the face count of cell p from
//              code[p]; per-workgroup vertex and face counts (wave ballots + popcount).
//   scan       one workgroup's exclusive scan of both count arrays; the totals go to counts[0] (V) and counts[1] (F).
//   vertices   vbase[p] = index of the first vertex of voxel p (workgroup offset + ballot rank), and the vertex rows < vertex_capacity.
//   faces      row of the first face of cell p (workgroup offset + ballot rank over the four bits of the face count); the index of an
//              edge's vertex is vbase[owner] + popcount(mask[owner] & bits below e); face rows < face_capacity.
//
// Workspace: four ints per workgroup (counts and offsets of vertices and faces), then vbase (4 bytes), code (2) and mask (1) per voxel;
// every slot is written before it is read, by the same call.
//
// Compiled with -ffp-contract=off and correctly rounded division (build.py): every product, sum and quotient of a vertex is rounded on
// its own, in the order um_tsdf_points (fusion.hip) and the host restatement of unimatch_amd/fusion.py evaluate them.
#include "common.h"
#include "timing.h"
#include "tsdf_grid.h"

extern void um_set_error(const char* fmt, ...);

#define UM_MESH_WG 256                         // threads = voxels per workgroup (four waves)
#define UM_MESH_SCAN_WG 1024                   // threads of the single scan workgroup (sixteen waves)

// ---- the six tetrahedra of a cell -------------------------------------------------------------------------------------------------

// corner q (0..3) of tetrahedron tau (0..5) as a corner mask of the cell: the permutations of (0, 1, 2) in lexicographic order
constexpr int tet_corner(int tau, int q) {
    const int p0 = tau >> 1;
    const int p1 = tau == 0 ? 1 : tau == 1 ? 2 : tau == 2 ? 0 : tau == 3 ? 2 : tau == 4 ? 0 : 1;
    return q == 0 ? 0 : q == 1 ? 1 << p0 : q == 2 ? (1 << p0) | (1 << p1) : 7;
}

constexpr bool tet_positive(int tau) { return tau == 0 || tau == 3 || tau == 4; }     // the sign of the permutation

// the edge between positions q < r of a tetrahedron, numbered 0..5: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
constexpr unsigned tet_edge(int q, int r) {
    const int a = q < r ? q : r, b = q < r ? r : q;
    return (unsigned)(a == 0 ? b - 1 : a == 1 ? b + 1 : 5);
}

// the faces of a tetrahedron whose corner q is inside iff bit q of `inside` is set, for a permutation of sign `positive`: bits 0..1 the
// number of triangles n, then six 3-bit edge numbers (tet_edge), three per triangle
constexpr unsigned tet_faces(int inside, bool positive) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
    int ni = 0, no = 0;
    for (int q = 0; q < 4; ++q) {
        if (inside >> q & 1) in[ni++] = q;
        else out[no++] = q;
    }
    unsigned e[6] = {0, 0, 0, 0, 0, 0};
    unsigned n = 0;
    bool reversed = false;
    if (ni == 1) {
        const int a = in[0];
        n = 1;
        e[0] = tet_edge(a, out[0]), e[1] = tet_edge(a, out[1]), e[2] = tet_edge(a, out[2]);
        reversed = positive == ((a & 1) == 1);
    } else if (ni == 3) {
        const int a = out[0];
        n = 1;
        e[0] = tet_edge(a, in[0]), e[1] = tet_edge(a, in[1]), e[2] = tet_edge(a, in[2]);
        reversed = !(positive == ((a & 1) == 1));
    } else if (ni == 2) {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        const unsigned q0 = tet_edge(a, c), q1 = tet_edge(a, d), q2 = tet_edge(b, d), q3 = tet_edge(b, c);
        n = 2;
        e[0] = q0, e[1] = q1, e[2] = q2, e[3] = q0, e[4] = q2, e[5] = q3;
        reversed = positive == (((a + b) & 1) == 0);
    }
    if (reversed) {
        unsigned t = e[0];
        e[0] = e[2], e[2] = t;
        t = e[3], e[3] = e[5], e[5] = t;
    }
    unsigned packed = n;
    for (int s = 0; s < 6; ++s) packed |= e[s] << (2 + 3 * s);
    return packed;
}

#define UM_TET_ROW(S) tet_faces(0, S), tet_faces(1, S), tet_faces(2, S), tet_faces(3, S), tet_faces(4, S), tet_faces(5, S),            \
                      tet_faces(6, S), tet_faces(7, S), tet_faces(8, S), tet_faces(9, S), tet_faces(10, S), tet_faces(11, S),         \
                      tet_faces(12, S), tet_faces(13, S), tet_faces(14, S), tet_faces(15, S)
// [sign of the permutation][inside pattern of the four corners]: evaluated by the compiler from the rules above
__constant__ const unsigned UM_TET_FACES[2][16] = {{UM_TET_ROW(false)}, {UM_TET_ROW(true)}};

// the inside pattern of tetrahedron TAU from the corner code of its cell
template <int TAU> __device__ __forceinline__ int tet_pattern(int code) {
    return (code & 1) | ((code >> tet_corner(TAU, 1) & 1) << 1) | ((code >> tet_corner(TAU, 2) & 1) << 2) | ((code >> 7 & 1) << 3);
}

template <int TAU> __device__ __forceinline__ int tet_face_count(int code) {
    const int n = __popc(tet_pattern<TAU>(code));
    return n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
}

// faces of cell p from its code: 0 for a code without the active bit
__device__ __forceinline__ int cell_face_count(int code) {
    if (!(code & 256)) return 0;
    return tet_face_count<0>(code) + tet_face_count<1>(code) + tet_face_count<2>(code) + tet_face_count<3>(code) +
           tet_face_count<4>(code) + tet_face_count<5>(code);
}

__device__ __forceinline__ void voxel_ijk(const TsdfGrid& g, long p, int& i, int& j, int& k) {
    const long row = p / g.nx;
    i = (int)(p - row * g.nx);
    k = (int)(row / g.ny);
    j = (int)(row - (long)k * g.ny);
}

// the linear offset of the corner / edge mask m: bit 0 = +x, bit 1 = +y, bit 2 = +z
__device__ __forceinline__ long mask_offset(const TsdfGrid& g, int m) {
    return (long)(m & 1) + (m & 2 ? (long)g.nx : 0L) + (m & 4 ? (long)g.nx * g.ny : 0L);
}

// ---- pass 1: the code of every cell -----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(UM_MESH_WG) void tsdf_mesh_cells_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                     unsigned short* __restrict__ code, TsdfGrid g, long total,
                                                                     float min_weight) {
    const long p = (long)blockIdx.x * UM_MESH_WG + threadIdx.x;
    if (p >= total) return;
    int i, j, k;
    voxel_ijk(g, p, i, j, k);
    const bool cell = i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz;
    int c = cell ? 256 : 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const long n = cell ? p + mask_offset(g, m) : p;      // a clamped (in-volume) address; the tap is discarded
        const float t = tsdf[n], w = weight[n];
        if (!tsdf_valid(t, w, min_weight)) c &= ~256;
        if (t < 0.f) c |= 1 << m;
    }
    code[p] = (unsigned short)(c & 256 ? c : 0);
}

// ---- pass 2: vertex masks, per-workgroup counts -----------------------------------------------------------------------------------

// the edges of voxel p that carry a vertex, bit e - 1 for edge e: a sign change in an active cell that contains the edge
__device__ __forceinline__ int vertex_mask(const unsigned short* __restrict__ code, const TsdfGrid& g, long p, int i, int j, int k,
                                           int& own) {
    int m = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const bool in = i >= (s & 1) && j >= (s >> 1 & 1) && k >= (s >> 2 & 1);
        const int cd = code[in ? p - mask_offset(g, s) : p];  // a clamped address; the code is discarded
        if (s == 0) own = cd;
        if (!in || !(cd & 256)) continue;
#pragma unroll
        for (int e = 1; e < 8; ++e)
            if (!(e & s) && ((cd >> s ^ cd >> (s | e)) & 1)) m |= 1 << (e - 1);
    }
    return m;
}

__global__ __launch_bounds__(UM_MESH_WG) void tsdf_mesh_classify_kernel(const unsigned short* __restrict__ code,
                                                                        unsigned char* __restrict__ mask, int* __restrict__ vcount,
                                                                        int* __restrict__ fcount, TsdfGrid g, long total) {
    __shared__ int wave_v[UM_MESH_WG / 64], wave_f[UM_MESH_WG / 64];
    const long p = (long)blockIdx.x * UM_MESH_WG + threadIdx.x;
    int m = 0, nf = 0;
    if (p < total) {
        int i, j, k, own;
        voxel_ijk(g, p, i, j, k);
        m = vertex_mask(code, g, p, i, j, k, own);
        nf = cell_face_count(own);
        mask[p] = (unsigned char)m;
    }
    int nv = 0, f = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) nv += __popcll(__ballot(m >> b & 1));
#pragma unroll
    for (int b = 0; b < 4; ++b) f += __popcll(__ballot(nf >> b & 1)) << b;      // a cell has at most 12 faces: four bits
    if ((threadIdx.x & 63) == 0) {
        wave_v[threadIdx.x >> 6] = nv;
        wave_f[threadIdx.x >> 6] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        vcount[blockIdx.x] = wave_v[0] + wave_v[1] + wave_v[2] + wave_v[3];
        fcount[blockIdx.x] = wave_f[0] + wave_f[1] + wave_f[2] + wave_f[3];
    }
}

// ---- pass 3: both exclusive scans -------------------------------------------------------------------------------------------------

// offsets[i] = counts[0] + ... + counts[i - 1] for both arrays, totals[0] / totals[1] the sums; one workgroup, each thread a contiguous
// run (the scan of tsdf_points_scan_kernel, twice)
__global__ __launch_bounds__(UM_MESH_SCAN_WG) void tsdf_mesh_scan_kernel(const int* __restrict__ vcount, const int* __restrict__ fcount,
                                                                         int* __restrict__ voffset, int* __restrict__ foffset,
                                                                         int* __restrict__ totals, int n) {
    __shared__ int wave_sum[2][UM_MESH_SCAN_WG / 64];
    const int per = (n + UM_MESH_SCAN_WG - 1) / UM_MESH_SCAN_WG;
    const long lo = (long)threadIdx.x * per;
    const long hi = lo + per < (long)n ? lo + per : (long)n;
    int sv = 0, sf = 0;
    for (long i = lo; i < hi; ++i) {
        sv += vcount[i];
        sf += fcount[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int iv = sv, jf = sf;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int uv = __shfl_up(iv, o, 64), uf = __shfl_up(jf, o, 64);
        iv = lane >= o ? iv + uv : iv;
        jf = lane >= o ? jf + uf : jf;
    }
    if (lane == 63) {
        wave_sum[0][wave] = iv;
        wave_sum[1][wave] = jf;
    }
    __syncthreads();
    int bv = 0, bf = 0;
    for (int q = 0; q < wave; ++q) {
        bv += wave_sum[0][q];
        bf += wave_sum[1][q];
    }
    int rv = bv + iv - sv, rf = bf + jf - sf;
    for (long i = lo; i < hi; ++i) {
        const int cv = vcount[i], cf = fcount[i];
        voffset[i] = rv;
        foffset[i] = rf;
        rv += cv;
        rf += cf;
    }
    if (threadIdx.x == UM_MESH_SCAN_WG - 1) {
        totals[0] = bv + iv;
        totals[1] = bf + jf;
    }
}

// ---- pass 4: vertex bases and vertex rows -----------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned char mesh_byte(float v) {
    return (unsigned char)fminf(fmaxf(v == v ? rintf(v) : 0.f, 0.f), 255.f);
}

__global__ __launch_bounds__(UM_MESH_WG) void tsdf_mesh_vertices_kernel(const float* __restrict__ tsdf, const float* __restrict__ color,
                                                                        const unsigned char* __restrict__ mask,
                                                                        const int* __restrict__ voffset, int* __restrict__ vbase,
                                                                        float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                        TsdfGrid g, long total, int capacity) {
    __shared__ int wave_n[UM_MESH_WG / 64];
    const long p = (long)blockIdx.x * UM_MESH_WG + threadIdx.x;
    const int m = p < total ? mask[p] : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n = 0, row = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const unsigned long long bal = __ballot(m >> b & 1);
        n += __popcll(bal);
        row += __popcll(bal & below);
    }
    if (lane == 0) wave_n[wave] = n;
    __syncthreads();
    if (p >= total) return;
    row += voffset[blockIdx.x];
    for (int q = 0; q < wave; ++q) row += wave_n[q];
    vbase[p] = row;
    if (!m) return;
    int i, j, k;
    voxel_ijk(g, p, i, j, k);
    const float base[3] = {g.ox + (float)i * g.voxel, g.oy + (float)j * g.voxel, g.oz + (float)k * g.voxel};
    const long planes = (long)g.nx * g.ny * g.nz;
    const float tp = tsdf[p];
#pragma unroll
    for (int e = 1; e < 8; ++e) {
        if (!(m >> (e - 1) & 1)) continue;
        if (row >= 0 && row < capacity) {
            const long n2 = p + mask_offset(g, e);            // inside the volume: the edge lies in an active cell
            const float s = tp / (tp - tsdf[n2]);
            float* o = xyz + (long)row * 3;
            o[0] = e & 1 ? base[0] + s * g.voxel : base[0];
            o[1] = e & 2 ? base[1] + s * g.voxel : base[1];
            o[2] = e & 4 ? base[2] + s * g.voxel : base[2];
            if (rgb) {
                unsigned char* q = rgb + (long)row * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float cp = color[ch * planes + p], cn = color[ch * planes + n2];
                    q[ch] = mesh_byte(cp + s * (cn - cp));
                }
            }
        }
        ++row;
    }
}

// ---- pass 5: face rows -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int pick6(unsigned id, const int (&v)[6]) {
    return id == 0 ? v[0] : id == 1 ? v[1] : id == 2 ? v[2] : id == 3 ? v[3] : id == 4 ? v[4] : v[5];
}

// the triangles of tetrahedron TAU of a cell into rows row.. (rows >= capacity are skipped); vb / mk: vertex base and vertex mask of
// the seven voxels cell + 0..6 that own the cell's edges
template <int TAU> __device__ __forceinline__ void tet_emit(int code, const int (&vb)[7], const int (&mk)[7], int* __restrict__ faces,
                                                            int& row, int capacity) {
    const unsigned packed = UM_TET_FACES[tet_positive(TAU) ? 1 : 0][tet_pattern<TAU>(code)];
    const int n = (int)(packed & 3u);
    if (n == 0) return;
    int v[6];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = q + 1; r < 4; ++r) {
            const int owner = tet_corner(TAU, q), e = tet_corner(TAU, r) ^ owner;
            v[tet_edge(q, r)] = vb[owner] + __popc(mk[owner] & ((1 << (e - 1)) - 1));
        }
    for (int t = 0; t < n; ++t) {
        if (row >= 0 && row < capacity) {
            int* o = faces + (long)row * 3;
            const unsigned tri = packed >> (2 + 9 * t);
            o[0] = pick6(tri & 7u, v);
            o[1] = pick6(tri >> 3 & 7u, v);
            o[2] = pick6(tri >> 6 & 7u, v);
        }
        ++row;
    }
}

__global__ __launch_bounds__(UM_MESH_WG) void tsdf_mesh_faces_kernel(const unsigned short* __restrict__ code,
                                                                     const unsigned char* __restrict__ mask,
                                                                     const int* __restrict__ vbase, const int* __restrict__ foffset,
                                                                     int* __restrict__ faces, TsdfGrid g, long total, int capacity) {
    __shared__ int wave_n[UM_MESH_WG / 64];
    const long p = (long)blockIdx.x * UM_MESH_WG + threadIdx.x;
    const int cd = p < total ? code[p] : 0;
    const int nf = cell_face_count(cd);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n = 0, row = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long bal = __ballot(nf >> b & 1);
        n += __popcll(bal) << b;
        row += __popcll(bal & below) << b;
    }
    if (lane == 0) wave_n[wave] = n;
    __syncthreads();
    if (!nf) return;
    row += foffset[blockIdx.x];
    for (int q = 0; q < wave; ++q) row += wave_n[q];
    int vb[7], mk[7];
#pragma unroll
    for (int m = 0; m < 7; ++m) {                             // an active cell: all its corners are inside the volume
        const long q = p + mask_offset(g, m);
        vb[m] = vbase[q];
        mk[m] = mask[q];
    }
    tet_emit<0>(cd, vb, mk, faces, row, capacity);
    tet_emit<1>(cd, vb, mk, faces, row, capacity);
    tet_emit<2>(cd, vb, mk, faces, row, capacity);
    tet_emit<3>(cd, vb, mk, faces, row, capacity);
    tet_emit<4>(cd, vb, mk, faces, row, capacity);
    tet_emit<5>(cd, vb, mk, faces, row, capacity);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------

static inline long mesh_groups(int nx, int ny, int nz) { return ((long)nx * ny * nz + UM_MESH_WG - 1) / UM_MESH_WG; }

extern "C" size_t um_tsdf_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (!tsdf_dims_ok(nx, ny, nz)) return 0;
    // vertex counts | face counts | vertex offsets | face offsets | vbase (int) | code (16 bits) | mask (8 bits)
    return (size_t)mesh_groups(nx, ny, nz) * 4 * sizeof(int) + (size_t)nx * ny * nz * (sizeof(int) + sizeof(unsigned short) + 1);
}

extern "C" int um_tsdf_mesh(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const float* origin,
                            float voxel, float min_weight, float* xyz, unsigned char* rgb, int* faces, int* counts, int vertex_capacity,
                            int face_capacity, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tsdf || !weight || !origin || !xyz || !faces || !counts || (color == nullptr) != (rgb == nullptr) || !tsdf_dims_ok(nx, ny, nz) ||
        vertex_capacity < 0 || face_capacity < 0 || !tsdf_positive(voxel) || min_weight != min_weight) {
        um_set_error("um_tsdf_mesh: bad argument (dims=%d x %d x %d vertex_capacity=%d face_capacity=%d voxel=%g min_weight=%g; "
                     "nx ny nz < 2^31; color and rgb go together)", nx, ny, nz, vertex_capacity, face_capacity, (double)voxel,
                     (double)min_weight);
        return UM_ERR_BAD_ARG;
    }
    const size_t need = um_tsdf_mesh_workspace_bytes(nx, ny, nz);
    if (!workspace || ws_bytes < need || (uintptr_t)workspace % sizeof(int) != 0) {
        um_set_error("um_tsdf_mesh: workspace of %zu bytes, %zu needed (4-byte aligned)", ws_bytes, need);
        return UM_ERR_WORKSPACE;
    }
    const TsdfGrid g = {nx, ny, nz, origin[0], origin[1], origin[2], voxel};
    const long total = (long)nx * ny * nz;
    const int n = (int)mesh_groups(nx, ny, nz);
    int* vcount = (int*)workspace;
    int* fcount = vcount + n;
    int* voffset = fcount + n;
    int* foffset = voffset + n;
    int* vbase = foffset + n;
    unsigned short* code = (unsigned short*)(vbase + total);
    unsigned char* mask = (unsigned char*)(code + total);
    const dim3 grid((unsigned)n), wg(UM_MESH_WG);
    ScopedKernelTimer timer(UM_K_CONVEX_UPSAMPLE, stream);
    hipLaunchKernelGGL(tsdf_mesh_cells_kernel, grid, wg, 0, stream, tsdf, weight, code, g, total, min_weight);
    hipLaunchKernelGGL(tsdf_mesh_classify_kernel, grid, wg, 0, stream, (const unsigned short*)code, mask, vcount, fcount, g, total);
    hipLaunchKernelGGL(tsdf_mesh_scan_kernel, dim3(1), dim3(UM_MESH_SCAN_WG), 0, stream, (const int*)vcount, (const int*)fcount, voffset,
                       foffset, counts, n);
    hipLaunchKernelGGL(tsdf_mesh_vertices_kernel, grid, wg, 0, stream, tsdf, color, (const unsigned char*)mask, (const int*)voffset, vbase,
                       xyz, rgb, g, total, vertex_capacity);
    hipLaunchKernelGGL(tsdf_mesh_faces_kernel, grid, wg, 0, stream, (const unsigned short*)code, (const unsigned char*)mask,
                       (const int*)vbase, (const int*)foffset, faces, g, total, face_capacity);
    return (int)hipGetLastError();
}
