// Stand-alone host check of csrc/r3d_resources.h on a machine WITHOUT a GPU, where every HIP create call fails cleanly: the
// failure paths of the owning types, the arena and the staging helpers, which cannot be provoked on a shared card.  Built with the host sanitizers and run by
// tools/cpu_sanitize_resources.sh; not a pytest.  With a GPU present it does nothing.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../3d_reconstruction_project_amd/csrc/r3d_internal.h"

// what api.hip supplies in the library
int r3d_fail(r3d_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}
void r3d_prof_harvest(r3d_ctx *, r3d_prof_set &) {}
bool r3d_roctx_push(const char *) { return false; }
void r3d_roctx_pop() {}

static int g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        g_checks++;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static bool counts_zero() {
    return r3d_live.device_allocs == 0 && r3d_live.device_bytes == 0 && r3d_live.pinned_allocs == 0 && r3d_live.events == 0 &&
           r3d_live.streams == 0;
}

int main() {
    if (access("/dev/kfd", F_OK) == 0) {
        printf("skipped: a GPU is present\n");
        return 0;
    }
    void *probe = nullptr;
    const hipError_t no_dev = hipMalloc(&probe, 16);
    if (no_dev == hipSuccess) {
        (void)hipFree(probe);
        printf("skipped: a GPU is present\n");
        return 0;
    }
    const std::string why = hipGetErrorString(no_dev);

    // a failed reserve under each policy: the buffer stays empty, R3D_E_OOM, the message of the parent code, nothing counted
    struct { const r3d_grow *g; const char *name; size_t want; const char *prefix; } pol[] = {
        {&R3D_GROW_WORKSPACE, "workspace", 1000 + 1000 / 8 + 4096, ""},
        {&R3D_GROW_MODEL, "model", 1000 + 1000 / 2 + 4096, ""},
        {&R3D_GROW_VOXEL_TABLE, "voxel table", 1000 + 1000 / 2 + 4096, ""},
        {&R3D_GROW_TSDF, "tsdf", 1000, "tsdf: "},
    };
    for (auto &q : pol) {
        r3d_ctx ctx;
        r3d_buf b;
        CHECK(b.reserve(&ctx, nullptr, 1000, *q.g, 0, q.g->alloc_first) == R3D_E_OOM);
        CHECK(b.p == nullptr && b.cap == 0);
        char want[256];
        snprintf(want, sizeof want, "%shipMalloc(%zu) failed: %s", q.prefix, q.want, why.c_str());
        CHECK(ctx.err == want);
        CHECK(counts_zero());
        CHECK(b.reserve(&ctx, nullptr, 0, *q.g) == R3D_OK);   // nothing to grow: no HIP call
        printf("reserve fails cleanly under the %s policy: %s\n", q.name, ctx.err.c_str());
    }
    {
        r3d_buf b;
        CHECK(b.alloc(64) != hipSuccess && b.p == nullptr && b.cap == 0);
        r3d_pinned h;
        CHECK(h.alloc(64, hipHostMallocMapped) != hipSuccess && h.p == nullptr);
        r3d_event e;
        CHECK(e.create() != hipSuccess && (hipEvent_t)e == nullptr);
        CHECK(e.create(hipEventDisableTiming) != hipSuccess && (hipEvent_t)e == nullptr);
        r3d_events<5> ring;
        CHECK(ring.create_all() != hipSuccess);
        for (int i = 0; i < 5; i++) CHECK(ring[i] == nullptr);
        r3d_stream s;
        CHECK(s.create(hipStreamNonBlocking) != hipSuccess && (hipStream_t)s == nullptr);
        CHECK(counts_zero());
    }
    printf("pinned, event, event-array and stream creation fail cleanly\n");

    // moves: the source ends empty, the handle arrives once.  The handles are made up (nothing can be allocated here) and taken
    // out again by hand before any destructor could pass them to HIP.
    {
        r3d_buf a;
        a.p = (void *)0x1000; a.cap = 64;
        r3d_buf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == (void *)0x1000 && b.cap == 64);
        r3d_buf c;
        c = std::move(b);
        CHECK(b.p == nullptr && b.cap == 0 && c.p == (void *)0x1000 && c.cap == 64);
        c.p = nullptr; c.cap = 0;

        r3d_pinned h;
        h.p = (void *)0x2000;
        r3d_pinned h2(std::move(h)), h3;
        h3 = std::move(h2);
        CHECK(h.p == nullptr && h2.p == nullptr && h3.p == (void *)0x2000);
        h3.p = nullptr;

        r3d_events<3> ev;
        ev.e[1] = (hipEvent_t)0x3000;
        r3d_events<3> ev2(std::move(ev)), ev3;
        ev3 = std::move(ev2);
        CHECK(ev[1] == nullptr && ev2[1] == nullptr && ev3[1] == (hipEvent_t)0x3000 && ev3[0] == nullptr);
        ev3.e[1] = nullptr;

        r3d_stream s;
        s.s = (hipStream_t)0x4000;
        r3d_stream s2(std::move(s)), s3;
        s3 = std::move(s2);
        CHECK((hipStream_t)s == nullptr && (hipStream_t)s2 == nullptr && (hipStream_t)s3 == (hipStream_t)0x4000);
        s3.s = nullptr;
        CHECK(counts_zero());
    }
    printf("moves leave the source empty\n");

    {
        std::vector<r3d_buf> v;
        for (int i = 0; i < 1000; i++) v.emplace_back();   // reallocates several times: needs the noexcept move
        CHECK(v.size() == 1000 && v[999].p == nullptr);
    }
    {
        r3d_ctx ctx;
        r3d_sgm_ws ws;
        DevArena cloud(&ctx), pp(&ctx, ctx.pp_bufs);
        CHECK(&cloud.bufs == &ctx.cloud_bufs && &pp.bufs == &ctx.pp_bufs);
    }
    printf("a vector of empty buffers, an empty context, a lane workspace and arenas are destroyed cleanly\n");

    for (int which = 0; which < 2; which++) {
        r3d_ctx ctx;
        DevArena ar(&ctx, which ? ctx.pp_bufs : ctx.cloud_bufs);
        CHECK(ar.get(100) == nullptr && ar.rc == R3D_E_OOM);
        CHECK(ar.bufs.size() == 1 && ar.bufs[0].p == nullptr && ar.bufs[0].cap == 0);
        ctx.err = "latched";
        CHECK(ar.get(100) == nullptr && ar.rc == R3D_E_OOM && ctx.err == "latched" && ar.bufs.size() == 1);
        // a poisoned context is refused before anything is reserved, for both lists
        r3d_ctx bad;
        bad.poisoned = true;
        DevArena ar2(&bad, which ? bad.pp_bufs : bad.cloud_bufs);
        CHECK(ar2.get(100) == nullptr && ar2.rc == R3D_E_HIP && ar2.bufs.empty());
        CHECK(bad.err.find("context poisoned") == 0);
    }
    CHECK(counts_zero());
    printf("an arena returns null and latches rc on a failed reserve and on a poisoned context\n");

    // the staging helpers of the host-buffer entry points (r3d_internal.h)
    {
        r3d_ctx ctx;
        DevArena ar(&ctx);
        const double *d = (const double *)0x1;
        CHECK(r3d_upload<double>(&ctx, ar, nullptr, 5, &d) == R3D_OK && d == nullptr && ar.next == 0 && ar.bufs.empty() && ctx.err.empty());
        double host[4] = {1, 2, 3, 4};
        CHECK(r3d_download<double>(&ctx, nullptr, (const double *)0x1000, 4) == R3D_OK);   // made-up device pointers: HIP must not see them
        CHECK(r3d_download<double>(&ctx, host, (const double *)0x1000, 0) == R3D_OK);
        CHECK(host[0] == 1 && host[3] == 4 && ctx.err.empty());
        CHECK(r3d_fits(&ctx, "who", "rows", 3, 3) == R3D_OK && ctx.err.empty());
        CHECK(r3d_fits(&ctx, "who", "rows", 4, 3) == R3D_E_BADARG && ctx.err == "who: 4 rows do not fit a capacity of 3");
        CHECK(counts_zero());
    }
    printf("a null upload takes no slot, a null or empty download does not reach HIP, r3d_fits refuses with the shared message\n");
    for (int plane = 0; plane < 2; plane++) {
        const uint16_t img[2 * 8] = {};
        const uint16_t *d = (const uint16_t *)0x1;
        uint16_t *dp = (uint16_t *)0x1;
        r3d_ctx ctx;
        DevArena ar(&ctx);
        const int rc = plane ? r3d_upload_plane(&ctx, ar, img, 5, 2, 8, &dp) : r3d_upload(&ctx, ar, img, 16, &d);
        CHECK(rc == R3D_E_OOM && ar.rc == R3D_E_OOM && ar.next == 1 && (plane ? dp == nullptr : d == nullptr));
        CHECK(ctx.err.find("hipMalloc(") == 0);
        ctx.err = "latched";
        CHECK((plane ? r3d_upload_plane(&ctx, ar, img, 5, 2, 8, &dp) : r3d_upload(&ctx, ar, img, 16, &d)) == R3D_E_OOM && ctx.err == "latched" && ar.next == 1);
        r3d_ctx bad;
        bad.poisoned = true;
        DevArena ar2(&bad);
        CHECK((plane ? r3d_upload_plane(&bad, ar2, img, 5, 2, 8, &dp) : r3d_upload(&bad, ar2, img, 16, &d)) == R3D_E_HIP);
        CHECK(ar2.bufs.empty() && bad.err.find("context poisoned") == 0 && (plane ? dp == nullptr : d == nullptr));
        CHECK(counts_zero());
    }
    printf("r3d_upload and r3d_upload_plane return the arena's latched failure and its refusal of a poisoned context\n");

    printf("resources_main: %d checks passed, all five counters zero throughout\n", g_checks);
    return 0;
}
