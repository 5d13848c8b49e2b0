"""What the triangle-mesh entry points refuse, and with which words: one table of (entry point, arguments, code, message) over the
host and the _dev forms of r3d_trimesh_smooth / _normals / _compact, r3d_trimesh_incidence / _adjacency, r3d_meshtopo_edges /
_components / _dedup and r3d_mesh_from_volume.  The checks behind these messages are shared code (csrc/r3d_internal.h: r3d_distinct,
r3d_fits, r3d_fits2; csrc/r3d_mesh.h: r3d_mesh_sizes_ok, r3d_mesh_empty_ok), so the table pins per entry point what a change
there could move: the text, the code, which of two refusals wins, and that a refused call writes nothing.  The messages are the
format strings of the sources with the entry point's name filled in.

The inputs are the four-vertex mesh and the two-unit volume of tests/test_staging_gpu.py; every case ends before or right after
its first kernel.  Output arrays start as 7 everywhere and are compared with 7 afterwards."""
import ctypes
import types

import numpy as np
import pytest

from tests.test_staging_gpu import TRUNC, VL, _mesh4, _protocol_mesh, _protocol_state

gpu = pytest.mark.gpu
_vp = ctypes.c_void_p
BADARG, UNSUPPORTED = -1, -4
INT32_MAX = 2 ** 31 - 1
COUNT = object()          # an int64 result, -1 before the call
OUTPUTS = ("oV", "oN", "oC", "oT", "tn", "vn", "off", "lst", "edg", "cnt", "lab", "ccnt", "area", "vmap", "orig")


def _arrays():
    vert, tri, nrm, col = _mesh4()
    bad, neg = tri.copy(), tri.copy()
    bad[1, 2], neg[0, 1] = 4, -1
    out = dict(oV=(4, 3, "f8"), oN=(4, 3, "f8"), oC=(4, 3, "f8"), oT=(2, 3, "i4"), tn=(2, 3, "f8"), vn=(4, 3, "f8"), off=(5, 1, "i4"),
               lst=(10, 1, "i4"), edg=(5, 2, "i4"), cnt=(5, 1, "i4"), lab=(2, 1, "i4"), ccnt=(1, 1, "i8"), area=(1, 1, "f8"), vmap=(4, 1, "i4"),
               orig=(2, 1, "i4"))
    assert tuple(out) == OUTPUTS
    a = dict(V=vert, N=nrm, C=col, T=tri, Tbad=bad, Tneg=neg)
    a.update({k: np.full((r, c), 7, t) for k, (r, c, t) in out.items()})
    return a


class _Buffers:
    """the arrays of one case by name, on the host or mirrored on the device"""

    def __init__(self, ctx, dev):
        self.ctx, self.host = ctx, _arrays()
        self.dev = {k: ctx.to_device(a) for k, a in self.host.items()} if dev else None

    def pointer(self, name):
        return _vp(self.dev[name]) if self.dev else self.host[name].ctypes.data_as(_vp)

    def outputs(self):
        if self.dev:
            for k in OUTPUTS:
                self.ctx.d2h(self.host[k], self.dev[k])
        return {k: self.host[k] for k in OUTPUTS}

    def free(self):
        if self.dev:
            self.ctx.sync()
            for d in self.dev.values():
                self.ctx.free(d)


# the arguments of every entry point from one set of named values; a string names an array of _Buffers
DEFAULTS = dict(nv=4, nt=2, V="V", N="N", C="C", T="T", flags=0, kind=1, scope=0, capv=4, capt=2, cap=0, ccap=0, oV="oV", oN="oN", oC="oC", oT="oT",
                tn="tn", vn="vn", off="off", lst="lst", edg="edg", cnt="cnt", lab="lab", ccnt="ccnt", area="area", vmap="vmap", orig="orig",
                vk=None, tk=None)
ARGS = {
    "r3d_trimesh_smooth": lambda a: (a.nv, a.nt, a.V, a.N, a.C, a.T, a.kind, 1, 0.5, -0.53, a.scope, a.oV, a.oN, a.oC),
    "r3d_trimesh_normals": lambda a: (a.nv, a.nt, a.V, a.T, a.flags, a.tn, a.vn),
    "r3d_trimesh_compact": lambda a: (a.nv, a.nt, a.V, a.N, a.C, a.T, a.vk, a.tk, a.flags, a.capv, a.capt, a.oV, a.oN, a.oC, a.oT, COUNT, COUNT),
    "r3d_trimesh_incidence": lambda a: (a.nv, a.nt, a.T, a.cap, a.off, a.lst, COUNT),
    "r3d_trimesh_adjacency": lambda a: (a.nv, a.nt, a.T, a.cap, a.off, a.lst, COUNT),
    "r3d_meshtopo_edges": lambda a: (a.nv, a.nt, a.T, a.cap, a.edg, a.cnt, None, COUNT),
    "r3d_meshtopo_components": lambda a: (a.nv, a.nt, a.V, a.T, a.ccap, a.lab, a.ccnt, a.area, COUNT),
    "r3d_meshtopo_dedup": lambda a: (a.nv, a.nt, a.V, a.N, a.C, a.T, a.flags, a.capv, a.capt, a.oV, a.oN, a.oC, a.oT, a.vmap, a.orig, COUNT, COUNT),
}
TWINS = ("r3d_trimesh_smooth", "r3d_trimesh_normals", "r3d_trimesh_compact", "r3d_meshtopo_components", "r3d_meshtopo_dedup")
NO_ARRAYS = dict(V=None, N=None, C=None, T=None, oV=None, oN=None, oC=None, oT=None, tn=None, vn=None, off=None, lst=None, edg=None, cnt=None,
                 lab=None, ccnt=None, area=None, vmap=None, orig=None)
MAX_T = INT32_MAX // 6

CASES = []   # (entry, dev, overrides, code, message, counts)


def _case(entry, overrides, code, message, counts=None, forms=None):
    """one row per form of the entry point; {who} is its name as the argument checks and the core print it: the trimesh twins share
    one, the meshtopo _dev forms carry the suffix"""
    for dev in forms if forms is not None else ((False, True) if entry in TWINS else (False,)):
        who = entry[4:] + ("_dev" if dev and entry.startswith("r3d_meshtopo") else "")
        CASES.append(pytest.param(entry + ("_dev" if dev else ""), dev, overrides, code, message and message.format(who=who), counts,
                                  id=f"{entry[4:]}{'_dev' if dev else ''}-{len(CASES)}"))


for _e in ARGS:
    _case(_e, dict(nv=-1), BADARG, "{who}: a negative count")
    _case(_e, dict(NO_ARRAYS, nv=INT32_MAX), UNSUPPORTED, "{who}: 2147483647 vertices do not fit int32 indices")
    _case(_e, dict(nt=MAX_T + 1), UNSUPPORTED, "{who}: 6 x 357913942 triangles do not fit int32 offsets")
    _case(_e, dict(T="Tbad", cap=10, ccap=1), BADARG, "{who}: a triangle index outside [0, 4)")
    _case(_e, dict(T="Tneg", cap=10, ccap=1), BADARG, "{who}: a triangle index outside [0, 4)")
    _case(_e, dict(nv=0, nt=1, cap=10, ccap=1), BADARG, "{who}: a triangle index outside [0, 0)")
# a missing required array
_case("r3d_trimesh_smooth", dict(V=None), BADARG, "trimesh_smooth: a missing array")
_case("r3d_trimesh_smooth", dict(oN=None), BADARG, "trimesh_smooth: a missing array")
_case("r3d_trimesh_normals", dict(T=None), BADARG, "trimesh_normals: a missing array")
for _e in ("r3d_trimesh_compact", "r3d_meshtopo_dedup"):
    _case(_e, dict(V=None), BADARG, "{who}: a missing array or a negative capacity")
    _case(_e, dict(oT=None), BADARG, "{who}: a missing array or a negative capacity")
for _e in ("r3d_trimesh_incidence", "r3d_trimesh_adjacency", "r3d_meshtopo_edges", "r3d_meshtopo_components"):
    _case(_e, dict(T=None), BADARG, "{who}: a missing array or a negative capacity")
_case("r3d_meshtopo_components", dict(ccap=1, area=None), BADARG, "{who}: a missing array or a negative capacity")
# an unknown flag bit (smooth: its two enumerations)
_case("r3d_trimesh_smooth", dict(kind=7), BADARG, "trimesh_smooth: unknown kind 7")
_case("r3d_trimesh_smooth", dict(scope=9), BADARG, "trimesh_smooth: unknown scope 9")
_case("r3d_trimesh_normals", dict(flags=2), BADARG, "trimesh_normals: unknown flags 2")
_case("r3d_trimesh_compact", dict(flags=8), BADARG, "trimesh_compact: unknown flags 8")
_case("r3d_meshtopo_dedup", dict(flags=4), BADARG, "{who}: unknown flags 4")
# the flags come ahead of a missing array, the limits ahead of the flags
_case("r3d_trimesh_compact", dict(flags=8, V=None), BADARG, "trimesh_compact: unknown flags 8")
_case("r3d_meshtopo_dedup", dict(flags=4, nv=-1), BADARG, "{who}: a negative count")
# overlaps (_dev forms): an output on an input, two outputs on one another, and the input named when both hold
for _e, _o in (("r3d_trimesh_smooth", "oV"), ("r3d_trimesh_normals", "vn"), ("r3d_trimesh_compact", "oV"), ("r3d_meshtopo_dedup", "oV")):
    _case(_e, {_o: "V"}, BADARG, _e[4:] + "_dev: an output array overlaps an input array", forms=(True,))
_case("r3d_meshtopo_components", dict(lab="T"), BADARG, "meshtopo_components_dev: an output array overlaps an input array", forms=(True,))
_case("r3d_trimesh_smooth", dict(oC="oN"), BADARG, "trimesh_smooth_dev: two output arrays overlap", forms=(True,))
_case("r3d_trimesh_normals", dict(tn="vn"), BADARG, "trimesh_normals_dev: two output arrays overlap", forms=(True,))
_case("r3d_trimesh_compact", dict(oN="oV"), BADARG, "trimesh_compact_dev: two output arrays overlap", forms=(True,))
_case("r3d_meshtopo_components", dict(ccap=1, area="ccnt"), BADARG, "meshtopo_components_dev: two output arrays overlap", forms=(True,))
_case("r3d_meshtopo_dedup", dict(orig="oT"), BADARG, "meshtopo_dedup_dev: two output arrays overlap", forms=(True,))
_case("r3d_trimesh_smooth", dict(oN="oV", oC="C"), BADARG, "trimesh_smooth_dev: two output arrays overlap", forms=(True,))
_case("r3d_trimesh_smooth", dict(oN="N", oC="oN"), BADARG, "trimesh_smooth_dev: an output array overlaps an input array", forms=(True,))
# the overlap comes after the missing array
_case("r3d_meshtopo_dedup", dict(oV="V", oT=None), BADARG, "meshtopo_dedup_dev: a missing array or a negative capacity", forms=(True,))
# capacities one row short: both counts in one message, whichever is short; a single quantity in r3d_fits' words
for _e in ("r3d_trimesh_compact", "r3d_meshtopo_dedup"):
    _case(_e, dict(capv=3), BADARG, "{who}: 4 vertices and 2 triangles do not fit capacities of 3 and 2")
    _case(_e, dict(capt=1), BADARG, "{who}: 4 vertices and 2 triangles do not fit capacities of 4 and 1")
    _case(_e, dict(capv=3, capt=1), BADARG, "{who}: 4 vertices and 2 triangles do not fit capacities of 3 and 1")
    _case(_e, dict(capv=0, capt=0), 0, None, counts=(4, 2))
_case("r3d_trimesh_incidence", dict(cap=5), BADARG, "trimesh_incidence: 6 entries do not fit a capacity of 5")
_case("r3d_trimesh_adjacency", dict(cap=9), BADARG, "trimesh_adjacency: 10 entries do not fit a capacity of 9")
_case("r3d_meshtopo_edges", dict(cap=4), BADARG, "meshtopo_edges: 5 edges do not fit a capacity of 4")
_case("r3d_trimesh_incidence", dict(cap=0), 0, None, counts=(6,))
_case("r3d_trimesh_adjacency", dict(cap=0), 0, None, counts=(10,))
_case("r3d_meshtopo_edges", dict(cap=0), 0, None, counts=(5,))


def _call(r3d, ctx, entry, args, code, message, counts):
    got = [ctypes.c_int64(-1) for a in args if a is COUNT]
    refs = iter(got)
    args = [ctypes.byref(next(refs)) if a is COUNT else a for a in args]
    if code == 0:
        ctx.call(entry, *args)
        assert tuple(g.value for g in got) == counts
        return
    with pytest.raises(r3d.R3DError) as e:
        ctx.call(entry, *args)
    assert (e.value.code, str(e.value)) == (code, f"{r3d._lib.ERR_NAMES[code]}: {message}")


@gpu
@pytest.mark.parametrize("entry, dev, overrides, code, message, counts", CASES)
def test_mesh_entry_point_refuses(r3d, entry, dev, overrides, code, message, counts):
    ctx = r3d.default_context()
    b = _Buffers(ctx, dev)
    try:
        named = {k: b.pointer(v) if isinstance(v, str) else v for k, v in dict(DEFAULTS, **overrides).items()}
        _call(r3d, ctx, entry, ARGS[entry[:-4] if dev else entry](types.SimpleNamespace(**named)), code, message, counts)
        for name, a in b.outputs().items():
            assert (a == 7).all(), f"{entry} wrote {name}"
    finally:
        b.free()


# ---- r3d_mesh_from_volume ----------------------------------------------------------------------------------------------------------
NV, NT = 512, 930    # the mesh of the two-unit volume (tests/tsdf_mesh_ref.py)
VOLUME_CASES = [
    ((NV, NT, "V", None, "T"), BADARG, "mesh_from_volume: a missing array or a negative capacity"),
    ((NV, NT, "V", "C", None), BADARG, "mesh_from_volume: a missing array or a negative capacity"),
    ((-1, NT, "V", "C", "T"), BADARG, "mesh_from_volume: a missing array or a negative capacity"),
    ((NV - 1, NT, "V", "C", "T"), BADARG, "mesh_from_volume: 512 vertices and 930 triangles do not fit capacities of 511 and 930"),
    ((NV, NT - 1, "V", "C", "T"), BADARG, "mesh_from_volume: 512 vertices and 930 triangles do not fit capacities of 512 and 929"),
    ((NV - 1, NT - 1, "V", "C", "T"), BADARG, "mesh_from_volume: 512 vertices and 930 triangles do not fit capacities of 511 and 929"),
    ((0, 0, None, None, None), 0, None),
]


@gpu
@pytest.mark.parametrize("dev", [False, True])
def test_mesh_from_volume_refuses(r3d, dev):
    want = _protocol_mesh()
    assert (len(want[0]), len(want[2])) == (NV, NT)
    ctx = r3d.default_context()
    entry = "r3d_mesh_from_volume" + ("_dev" if dev else "")
    host = dict(V=np.full((NV, 3), 7.0), C=np.full((NV, 3), 7.0), T=np.full((NT, 3), 7, np.int32))
    d_out = {k: ctx.to_device(a) for k, a in host.items()} if dev else None
    try:
        with r3d.ScalableTSDFVolume(VL, TRUNC, r3d.TSDFVolumeColorType.RGB8, initial_units=2) as volume:
            volume.load_units(*_protocol_state())
            for (capv, capt, *names), code, message in VOLUME_CASES:
                ptrs = [None if k is None else _vp(d_out[k]) if dev else host[k].ctypes.data_as(_vp) for k in names]
                _call(r3d, ctx, entry, (volume._h, capv, capt, *ptrs, COUNT, COUNT), code, message, (NV, NT))
        for k, a in host.items():
            if dev:
                ctx.d2h(a, d_out[k])
            assert (a == 7).all(), f"{entry} wrote {k}"
    finally:
        if dev:
            ctx.sync()
            for d in d_out.values():
                ctx.free(d)
