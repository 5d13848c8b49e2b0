// Internal (not installed): what the entry points that take or produce a triangle mesh share on the host side -- the size limits,
// the empty-mesh refusal, and a mesh's arrays as one pair of structs with their staging ("Staging").  A new mesh
// entry point starts from here.
#pragma once
#include "r3d_internal.h"

// the size limits of the triangle-mesh entry points, the poisoned-context refusal included
static inline int r3d_mesh_sizes_ok(r3d_ctx *ctx, const char *who, int64_t nv, int64_t nt) {
    if (nv < 0 || nt < 0) return r3d_fail(ctx, R3D_E_BADARG, "%s: a negative count", who);
    if (nv > INT32_MAX - 1) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: %lld vertices do not fit int32 indices", who, (long long)nv);
    if (nt > (int64_t)INT32_MAX / 6) return r3d_fail(ctx, R3D_E_UNSUPPORTED, "%s: 6 x %lld triangles do not fit int32 offsets", who, (long long)nt);
    if (ctx->poisoned) return r3d_fail(ctx, R3D_E_HIP, "%s: context poisoned by an earlier timed-out call: destroy it", who);
    return R3D_OK;
}

// triangles without vertices: every corner is out of range, and no kernel is needed to say so
static inline int r3d_mesh_empty_ok(r3d_ctx *ctx, const char *who, int64_t nv, int64_t nt) {
    return nv == 0 && nt > 0 ? r3d_fail(ctx, R3D_E_BADARG, "%s: a triangle index outside [0, 0)", who) : R3D_OK;
}

// a mesh's arrays, all on the host or all on the device: [nv][3] rows of pos / nrm / col (nrm and col may be null), [nt][3] corners
struct r3d_mesh_in { const double *pos, *nrm, *col; const int32_t *tri; };
struct r3d_mesh_out { double *pos, *nrm, *col; int32_t *tri; };

// host arrays -> fresh arena buffers, in the order pos, nrm, col, tri; an absent array stays null and takes no slot
static inline int r3d_mesh_upload(r3d_ctx *ctx, DevArena &ar, const r3d_mesh_in &h, int64_t nv, int64_t nt, r3d_mesh_in *d) {
    const size_t n3 = (size_t)nv * 3;
    int rc;
    if ((rc = r3d_upload(ctx, ar, h.pos, n3, &d->pos)) || (rc = r3d_upload(ctx, ar, h.nrm, n3, &d->nrm)) || (rc = r3d_upload(ctx, ar, h.col, n3, &d->col)))
        return rc;
    return r3d_upload(ctx, ar, h.tri, (size_t)nt * 3, &d->tri);
}
// arena outputs as large as the inputs (a clean-up's counts are not known yet): positions always, normals and colours where the
// input has them, triangles when asked for.  The caller tests ar.rc after its last buffer.
static inline void r3d_mesh_outputs(DevArena &ar, const r3d_mesh_in &d_in, int64_t nv, int64_t nt, bool triangles, r3d_mesh_out *d) {
    const size_t bytes = (size_t)nv * 24;
    d->pos = (double *)ar.get(bytes);
    d->nrm = d_in.nrm ? (double *)ar.get(bytes) : nullptr;
    d->col = d_in.col ? (double *)ar.get(bytes) : nullptr;
    d->tri = triangles ? (int32_t *)ar.get((size_t)nt * 12) : nullptr;
}
// rows_v rows of every vertex attribute there is and rows_t triangles -> the caller's host arrays; enqueues only
static inline int r3d_mesh_download(r3d_ctx *ctx, const r3d_mesh_out &h, const r3d_mesh_out &d, int64_t rows_v, int64_t rows_t) {
    const size_t k3 = (size_t)rows_v * 3;
    int rc;
    if ((rc = r3d_download(ctx, h.pos, (const double *)d.pos, k3)) || (rc = r3d_download(ctx, h.nrm, (const double *)d.nrm, d.nrm ? k3 : 0)) ||
        (rc = r3d_download(ctx, h.col, (const double *)d.col, d.col ? k3 : 0)))
        return rc;
    return r3d_download(ctx, h.tri, (const int32_t *)d.tri, d.tri ? (size_t)rows_t * 3 : 0);
}
