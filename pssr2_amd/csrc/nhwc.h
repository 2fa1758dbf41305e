// NHWC tensor slices, their checks and the storage-type dispatch shared by the pointwise / per-channel kernel files.
#pragma once
#include "common.h"

namespace {   // internal linkage, as the kernels that take these by value

struct Ref { const void* p; int cs, co; };   // NHWC tensor slice: base, channel stride, channel offset
struct MRef { void* p; int cs, co; };

template <typename T> __device__ __forceinline__ const T* at(const Ref& r, long pix, int c) { return (const T*)r.p + pix * r.cs + r.co + c; }
template <typename T> __device__ __forceinline__ T* at(const MRef& r, long pix, int c) { return (T*)r.p + pix * r.cs + r.co + c; }

// flat index of an n x h x w pixel grid -> (image, row, column)
struct PixPos { long img; int y, x; };
__device__ __forceinline__ PixPos split_pix(long pix, int h, int w) {
    PixPos p;
    p.x = (int)(pix % w); pix /= w;
    p.y = (int)(pix % h);
    p.img = pix / h;
    return p;
}

}  // namespace

// runs CALL with T = the storage type of `dtype`
#define DISPATCH_T(dtype, CALL)                                             \
    do {                                                                    \
        if ((dtype) == PSSR_BF16) { using T = bf16_t; CALL; }               \
        else if ((dtype) == PSSR_F16) { using T = f16_t; CALL; }            \
        else if ((dtype) == PSSR_F32) { using T = float; CALL; }            \
        else { pssr_set_error("bad dtype %d", (dtype)); return PSSR_ERR_ARG; } \
    } while (0)

#define CHECK_REF(name, cs, co, c)                                                                               \
    PSSR_CHECK((cs) % 4 == 0 && (co) % 4 == 0 && (co) + (c) <= (cs), PSSR_ERR_ARG, name ": bad channel stride/offset (%d,%d,%d)", cs, co, c)

// the slice of a scalar kernel: any offset (the engines pass unaligned chunk offsets), inside its stride
#define CHECK_SLICE(name, cs, co, c)                                                                             \
    PSSR_CHECK((c) > 0 && (co) >= 0 && (long)(co) + (c) <= (long)(cs), PSSR_ERR_ARG, name ": channel slice outside its stride (%d,%d,%d)", cs, co, c)

#define CHECK_DTYPE(name, dtype) \
    PSSR_CHECK((dtype) == PSSR_BF16 || (dtype) == PSSR_F16 || (dtype) == PSSR_F32, PSSR_ERR_ARG, name ": bad dtype %d", dtype)
