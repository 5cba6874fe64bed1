// bbo_wave.hpp -- the wavefront and workgroup primitives every kernel header shares: the hand-over
// point inside one wavefront, the stop test of a population, the butterfly reductions over a lane
// group and the reductions of a workgroup through one LDS slot per wavefront.  Every engine is
// pinned bit for bit to its goldens, so a reduction that adds in another order (eig_wave_sum,
// sep_wave_sum, block_sum_1024) is a primitive of its own and stays with its kernels.
#pragma once

#include <hip/hip_runtime.h>

namespace bbo {

// hand-over point between the lanes of ONE wavefront (single-wavefront bodies: the hardware
// keeps a wavefront's memory operations in order, the fence stops the compiler from moving
// loads across the point)
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// run() launches with honor_stop: a population that has stopped takes no further generation
template<class C, class S>
__device__ inline bool pop_frozen(const C &c, const S *sc)
{
    return c.honor_stop && sc->stop != 0;
}

// DPP move of a 32-bit word / an fp64 value with control word CTRL, all rows and banks enabled.
// mov_dpp with bound_ctrl set instead of update_dpp(old = 0, ..., bound_ctrl = false): a lane whose
// source does not exist (the lanes row_shr shifts in) or is switched off reads 0 in the first form
// and keeps old = 0 in the second -- the same value -- and with row_mask = bank_mask = 0xf no lane
// is left out of the write, so `old` shows nowhere else.  But `old = 0` is an operand the compiler
// has to put into the destination first: a v_mov_b32 v, 0 in front of every v_mov_b32_dpp, twice
// per fp64 value, on the pipe the fp64 MFMAs share.  (A move under a partial row or bank mask does
// keep `old` in the lanes it leaves out and cannot take this form; there is none in the library.)
template<int CTRL>
__device__ inline int dpp_mov(int v)
{
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true);
}

template<int CTRL>
__device__ inline double dpp_mov(double v)
{
    const int lo = dpp_mov<CTRL>(__double2loint(v)), hi = dpp_mov<CTRL>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// an fp64 value of another lane of the wavefront through the LDS crossbar (ds_bpermute: not an
// instruction of the vector pipe); byte = 4 * the source lane, computed once by the caller
__device__ inline double lane_read64(double v, int byte)
{
    const int lo = __builtin_amdgcn_ds_bpermute(byte, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(byte, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// xor butterfly over G lanes (a power of two, <= 64, contiguous in one wavefront): every lane of
// the group returns the total
template<int G>
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

template<int G>
__device__ inline double group_prod(double v)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v *= __shfl_xor(v, off, G);
    return v;
}

// (v, s) of the minimum / maximum over a wavefront, on a tie the lower s
__device__ inline void wave_argmin(double &v, int &s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int os = __shfl_xor(s, off, 64);
        if (ov < v || (ov == v && os < s)) {
            v = ov;
            s = os;
        }
    }
}
__device__ inline void wave_argmax(double &v, int &s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int os = __shfl_xor(s, off, 64);
        if (ov > v || (ov == v && os < s)) {
            v = ov;
            s = os;
        }
    }
}

// Sum over a workgroup of NW wavefronts through scratch[NW] in LDS, the total in every thread.
// The first barrier lets a caller reuse the scratch of an earlier reduction.  The slots are added
// from left to right; the finish kernels that add them in pairs, (0 + 1) + (2 + 3), or reduce
// several values behind one pair of barriers keep their own form.
template<int NW>
__device__ inline double block_sum(double v, double *scratch)
{
    const int tid = threadIdx.x;
    v = group_sum<64>(v);
    __syncthreads();
    if ((tid & 63) == 0) scratch[tid >> 6] = v;
    __syncthreads();
    double s = scratch[0];
#pragma unroll
    for (int w = 1; w < NW; w++) s += scratch[w];
    return s;
}

// arg-min (SIGN = +1) or arg-max (SIGN = -1) with first-index tie-break over 256 threads
template<int SIGN>
__device__ inline void block_arg(double &v, int &idx, double *sval, int *sidx)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        const bool take = SIGN > 0 ? (ov < v || (ov == v && oi < idx))
                                   : (ov > v || (ov == v && oi < idx));
        if (take) {
            v = ov;
            idx = oi;
        }
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        sval[tid >> 6] = v;
        sidx[tid >> 6] = idx;
    }
    __syncthreads();
    v = sval[0];
    idx = sidx[0];
    for (int w = 1; w < 4; w++) {
        const bool take = SIGN > 0 ? (sval[w] < v || (sval[w] == v && sidx[w] < idx))
                                   : (sval[w] > v || (sval[w] == v && sidx[w] < idx));
        if (take) {
            v = sval[w];
            idx = sidx[w];
        }
    }
}

} // namespace bbo
