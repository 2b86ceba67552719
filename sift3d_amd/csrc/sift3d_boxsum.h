// sift3d_boxsum.h -- the windowed-sum tile core of the local cross-correlation kernels (sift3d_lncc.hip; contract:
// include/sift3d_amd.h, "Local cross-correlation", "Window sums").
//
// box(t)(p) is the sum of a per-voxel double t over the (2R + 1)^3 window around p clipped to the grid, formed
// separably in an order that is part of the contract: the x sums over the offsets -R .. R ascending, the y sums of
// those ascending, the z sums of those ascending, every sum from +0.0, an off-grid position adding +0.0, unfused.
//
// A 256-lane workgroup owns a 64 x 4 RY (x, y) tile (RY rows per lane: 1, or 2 for the 64 x 8 tile) and marches up a
// stretch of z.  Per plane:
//   1. the tile and its halo of R voxels are staged in LDS in the policy's RAW form (what lies in global memory: 3
//      floats per voxel for the statistics, 4 doubles for the force), component-planar, so that a wave's accesses fall
//      on consecutive addresses; an off-grid voxel is staged as zeros, which every policy expands to +0.0;
//   2. lane (lx, ly) forms the x sums of the rows ly, ly + 4, ... of the tile + halo: 2R + 1 raw reads per component,
//      expanded to the NQ doubles (the products are formed here, exactly, from the promoted floats) and added
//      ascending; the sums go to LDS as doubles (8-byte accesses, a wave on consecutive addresses);
//   3. the lane adds the 2R + 1 x sums of its column ascending in y: the plane sum of its column.
// The lane keeps the last 2R + 1 plane sums of its column (of each of its RY columns) in a ring of registers and, for
// the output plane R planes back, adds them in ascending z.  (A running sum that adds the new plane and subtracts the oldest would round
// differently; the contract is the plain sum.)  The ring is indexed at compile time: the march is unrolled by the
// 2R + 1 phases of the ring, which is why R is a template parameter.
#ifndef SIFT3D_BOXSUM_H
#define SIFT3D_BOXSUM_H

#include "sift3d_kernels_common.h"

constexpr int BOX_TX = 64;                       // a wave per row, as k_demons_force; a tile is BOX_TX x 4 RY

// A policy P states what is summed:
//   NQ, NRAW, raw_t          the doubles per voxel, and the components (of type raw_t) it keeps per voxel in LDS
//   load(x, y, z, raw)       the raw components of an on-grid voxel, from global memory
//   expand(raw, q)           the NQ doubles of a voxel from its raw components; all-zero raw gives NQ times +0.0
// box_march<P, R, RY>(pol, x0, y0, zlo, zhi, nx, ny, nz, lds, emit) calls emit(x, y, z, on_grid, sums) for every
// lane, each of its RY rows (y0 + ly + 4 i: a lane owns RY columns and keeps a ring for each) and every output plane
// zlo <= z < zhi of the 64 x 4 RY tile at (x0, y0); every lane of the workgroup must call it.
// LDS: raw raw_t [NRAW][4 RY + 2R][BOX_TX + 2R], x double [NQ][4 RY + 2R][BOX_TX].
template <class P, int R, int RY> struct BoxLds {
    static constexpr int W = 2 * R + 1, TY = 4 * RY, HX = BOX_TX + 2 * R, HY = TY + 2 * R;
    typename P::raw_t raw[P::NRAW][HY][HX];
    double x[P::NQ][HY][BOX_TX];
};

template <class P, int R, int RY, class Emit>
__device__ __forceinline__ void box_march(const P &pol, int x0, int y0, int zlo, int zhi, int nx, int ny, int nz,
                                          BoxLds<P, R, RY> &s, Emit &&emit)
{
    constexpr int NQ = P::NQ, NRAW = P::NRAW;
    constexpr int W = BoxLds<P, R, RY>::W, HX = BoxLds<P, R, RY>::HX, HY = BoxLds<P, R, RY>::HY;
    typedef typename P::raw_t raw_t;
    const int lx = (int)(threadIdx.x & 63), ly = (int)(threadIdx.x >> 6);
    double ring[RY][W][NQ];
#pragma unroll
    for (int ry = 0; ry < RY; ry++)
#pragma unroll
        for (int i = 0; i < W; i++)
#pragma unroll
            for (int k = 0; k < NQ; k++)
                ring[ry][i][k] = 0.0;
    // planes zlo - R .. zhi + R - 1 enter the ring; plane zp completes the window of output plane zp - R
    for (int zb = zlo - R; zb < zhi + R; zb += W) {
#pragma unroll
        for (int ph = 0; ph < W; ph++) {
            const int zp = zb + ph;
            if (zp >= zhi + R)                                               // uniform over the workgroup
                break;
            if (zp < 0 || zp >= nz) {                                        // an off-grid plane adds +0.0
#pragma unroll
                for (int ry = 0; ry < RY; ry++)
#pragma unroll
                    for (int k = 0; k < NQ; k++)
                        ring[ry][ph][k] = 0.0;
            } else {
                __syncthreads();                                             // the plane before has been read
                for (int i = (int)threadIdx.x; i < HY * HX; i += 256) {
                    const int hy = i / HX, hx = i - hy * HX;
                    const int gx = x0 - R + hx, gy = y0 - R + hy;
                    raw_t r[NRAW];
#pragma unroll
                    for (int k = 0; k < NRAW; k++)
                        r[k] = (raw_t)0;
                    if (gx >= 0 && gx < nx && gy >= 0 && gy < ny)
                        pol.load(gx, gy, zp, r);
#pragma unroll
                    for (int k = 0; k < NRAW; k++)
                        s.raw[k][hy][hx] = r[k];
                }
                __syncthreads();
                for (int hy = ly; hy < HY; hy += 4) {
                    double a[NQ];
#pragma unroll
                    for (int k = 0; k < NQ; k++)
                        a[k] = 0.0;
#pragma unroll
                    for (int j = 0; j < W; j++) {
                        raw_t r[NRAW];
                        double q[NQ];
#pragma unroll
                        for (int k = 0; k < NRAW; k++)
                            r[k] = s.raw[k][hy][lx + j];
                        pol.expand(r, q);
#pragma unroll
                        for (int k = 0; k < NQ; k++)
                            a[k] = a[k] + q[k];
                    }
#pragma unroll
                    for (int k = 0; k < NQ; k++)
                        s.x[k][hy][lx] = a[k];
                }
                __syncthreads();
#pragma unroll
                for (int ry = 0; ry < RY; ry++)
#pragma unroll
                    for (int k = 0; k < NQ; k++) {
                        double a = 0.0;
#pragma unroll
                        for (int j = 0; j < W; j++)
                            a = a + s.x[k][ly + 4 * ry + j][lx];
                        ring[ry][ph][k] = a;
                    }
            }
            const int z = zp - R;
            if (z >= zlo) {
#pragma unroll
                for (int ry = 0; ry < RY; ry++) {
                    double t[NQ];
#pragma unroll
                    for (int k = 0; k < NQ; k++) {
                        double a = 0.0;
#pragma unroll
                        for (int j = 1; j <= W; j++)                         // the oldest plane first: ascending z
                            a = a + ring[ry][(ph + j) % W][k];
                        t[k] = a;
                    }
                    const int x = x0 + lx, y = y0 + ly + 4 * ry;
                    emit(x, y, z, x < nx && y < ny, t);
                }
            }
        }
    }
}

#endif
