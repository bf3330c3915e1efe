// The argument checks that the entry points of more than one translation unit make, each stated once.  `what` is the entry
// point's name (its __func__); RN_OK, or rn_set_error's RN_E_INVALID with the message set, so a call site may join several
// with || and return RN_E_INVALID.  Checks of one family of entries stay with it (the ray caster's: raycast_common.h).
#pragma once
#include "rn_common.h"
#include <initializer_list>

constexpr int kMaxBatch = 65535;          // blockIdx.y or .z carries the item

static inline int rn_check_batch_sign(const char* what, int B)
{
    return B < 0 ? rn_set_error(RN_E_INVALID, "%s: B=%d", what, B) : RN_OK;
}

static inline int rn_check_batch_size(const char* what, int B)
{
    return B > kMaxBatch ? rn_set_error(RN_E_INVALID, "%s: B=%d (at most %d per call)", what, B, kMaxBatch) : RN_OK;
}

static inline int rn_check_batch(const char* what, int B)           // both at once, for an entry that returns early on B = 0
{
    return (B < 0 || B > kMaxBatch) ? rn_set_error(RN_E_INVALID, "%s: B=%d (0..%d per call)", what, B, kMaxBatch) : RN_OK;
}

// the sides the voxel and mesh tools are instantiated for; the ray caster also takes 96 (rn_check_grid_side_x32)
static inline int rn_check_grid_side_pow2(const char* what, int S)
{
    return (S != 32 && S != 64 && S != 128) ? rn_set_error(RN_E_INVALID, "%s: S=%d (32, 64 or 128)", what, S) : RN_OK;
}

static inline int rn_check_pointers(const char* what, std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if (!p) return rn_set_error(RN_E_INVALID, "%s: null pointer", what);
    return RN_OK;
}

// `bytes` is a power of two; a null pointer passes (whether it may be null is rn_check_pointers' question)
static inline int rn_check_aligned(const char* what, const void* p, int bytes, const char* name)
{
    return ((uintptr_t)p & (uintptr_t)(bytes - 1)) != 0 ? rn_set_error(RN_E_INVALID, "%s: %s must be %d-byte aligned", what, name, bytes)
                                                        : RN_OK;
}

// the frame of the integer camera and a window inside it, with the batch: what the carve and the pose search are given
static inline int rn_check_frame(const char* what, int B, int N, int f, int row0, int col0, int ph, int pw)
{
    if (rn_check_batch(what, B)) return RN_E_INVALID;
    if (N < 1 || N > 256 || f < 1 || f > 16 || f * N > 2048)
        return rn_set_error(RN_E_INVALID, "%s: N=%d, pixels_per_cell=%d (N <= 256, f <= 16, f N <= 2048)", what, N, f);
    const int side = f * N;
    if (ph < 1 || pw < 1 || row0 < 0 || col0 < 0 || row0 > side - ph || col0 > side - pw)
        return rn_set_error(RN_E_INVALID, "%s: window (%d, %d, %d, %d) outside the %d x %d frame", what, row0, col0, ph, pw, side, side);
    return RN_OK;
}

// the workspace of an entry whose rn_*_workspace_bytes gives `need`
static inline int rn_check_ws(const char* what, const void* ws, size_t ws_bytes, size_t need)
{
    if (rn_check_pointers(what, {ws}) || rn_check_aligned(what, ws, 16, "the workspace")) return RN_E_INVALID;
    return ws_bytes < need ? rn_set_error(RN_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need) : RN_OK;
}
