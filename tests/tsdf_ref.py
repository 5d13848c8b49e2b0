"""numpy restatement of the TSDF volume contract ("TSDF volume"): Open3D's ScalableTSDFVolume as recalled
from 0.18 (ScalableTSDFVolume.cpp, UniformTSDFVolume.cpp), written from the contract and not from the kernels.  Two forms of
every stage: a vectorised one (all touched units at once, one z step at a time) and a literal per-voxel loop for tiny volumes;
tests/test_tsdf_ref.py holds them equal bit for bit.  float32 arithmetic is numpy float32 (no fused multiply-add, correctly
rounded divide and square root); every sum is written in the order the contract gives.

The choices of Open3D that are not the obvious ones are named:"""
import numpy as np

QUIRK_TSDF_MATVEC_ORDER = True           # camera point = ((E0 x + E1 y) + E2 z) + E3 in float32, left to right
QUIRK_TSDF_Z_RUNNING_SUM = True          # the camera point of voxel z + 1 is that of z plus f32(E[k][2] * f32(vl)): a running sum
QUIRK_TSDF_NORMAL_IGNORES_WEIGHT = True  # the normal's trilinear values read tsdf alone: a never-observed voxel counts as 0.0

R = 16
f32 = np.float32
_LIMIT = 1 << 20
_CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))


def affine_inverse(E):
    """-> A^-1 (3x3 as nested floats), -A^-1 t: the inverse of [A t; 0 0 0 1] by the adjugate, in a fixed expression order"""
    E = np.asarray(E, dtype=np.float64)
    a, b, c, d, e, f, g, h, i = (float(E[r, k]) for r in range(3) for k in range(3))
    det = (a * (e * i - f * h) + b * (f * g - d * i)) + c * (d * h - e * g)
    adj = (e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d)
    Ai = [[adj[r * 3 + k] / det for k in range(3)] for r in range(3)]
    t = [float(E[k, 3]) for k in range(3)]
    ti = [-((Ai[k][0] * t[0] + Ai[k][1] * t[1]) + Ai[k][2] * t[2]) for k in range(3)]
    return Ai, ti


def depth_from_u16(raw, depth_scale, depth_trunc):
    z = np.asarray(raw).astype(f32) / f32(depth_scale)
    return np.where(z > f32(depth_trunc), f32(0), z).astype(f32)


class Volume:
    """units: {(X, Y, Z): [tsdf f32[16,16,16], weight f32[16,16,16], colour f64[3,16,16,16] or None]} indexed [x][y][z]"""

    def __init__(self, voxel_length, sdf_trunc, color=True, stride=4):
        self.vl, self.trunc, self.color, self.stride = float(voxel_length), float(sdf_trunc), bool(color), int(stride)
        self.ul = self.vl * R
        self.units = {}
        self.touched = []

    # ---- touch ----------------------------------------------------------------------------------------------------------------
    def touch(self, depth, cam, extrinsic):
        """-> sorted list of the unit indices the frame touches"""
        fx, fy, cx, cy = (float(v) for v in cam)
        Ai, ti = affine_inverse(extrinsic)
        H, W = depth.shape
        i, j = np.meshgrid(np.arange(0, H, self.stride), np.arange(0, W, self.stride), indexing="ij")
        z = depth[i, j].astype(np.float64)
        ok = z > 0
        i, j, z = i[ok].astype(np.float64), j[ok].astype(np.float64), z[ok]
        x, y = ((j - cx) * z) / fx, ((i - cy) * z) / fy
        lo, hi = [], []
        for k in range(3):
            p = ((Ai[k][0] * x + Ai[k][1] * y) + Ai[k][2] * z) + ti[k]
            lo.append(np.floor((p - self.trunc) / self.ul))
            hi.append(np.floor((p + self.trunc) / self.ul))
        boxes = np.unique(np.stack(lo + hi, 1).astype(np.int64), axis=0) if len(z) else np.zeros((0, 6), np.int64)
        if len(boxes) and (boxes[:, :3].min() < -_LIMIT or boxes[:, 3:].max() >= _LIMIT):
            raise OverflowError("unit index outside +-2^20")
        out = set()
        for b in boxes:
            for X in range(b[0], b[3] + 1):
                for Y in range(b[1], b[4] + 1):
                    for Z in range(b[2], b[5] + 1):
                        out.add((X, Y, Z))
        return sorted(out)

    def _new_unit(self):
        return [np.zeros((R, R, R), f32), np.zeros((R, R, R), f32), np.zeros((3, R, R, R), np.float64) if self.color else None]

    # ---- integrate ------------------------------------------------------------------------------------------------------------
    def integrate(self, depth, color, cam, extrinsic, literal=False):
        """depth float32 [H,W] metres (0: no sample); color uint8 [H,W,3] (ignored without colour); extrinsic world -> camera"""
        depth = np.ascontiguousarray(depth, dtype=f32)
        self.touched = self.touch(depth, cam, extrinsic)
        for key in self.touched:
            if key not in self.units:
                self.units[key] = self._new_unit()
        if not self.touched:
            return
        (self._integrate_literal if literal else self._integrate_vectorised)(depth, color, cam, np.asarray(extrinsic, dtype=np.float64))

    def _frame_constants(self, depth, cam, E):
        H, W = depth.shape
        fxf, fyf, cxf, cyf = (f32(v) for v in cam)
        return dict(Ef=E.astype(f32), fxf=fxf, fyf=fyf, cxf=cxf, cyf=cyf, ifx=f32(1) / fxf, ify=f32(1) / fyf, vlf=f32(self.vl),
                    truncf=f32(self.trunc), itrunc=f32(1) / f32(self.trunc), wlim=f32(W - 0.0001), hlim=f32(H - 0.0001))

    @staticmethod
    def _matvec(Ef, k, Px, Py, Pz):
        if QUIRK_TSDF_MATVEC_ORDER:
            return ((Ef[k, 0] * Px + Ef[k, 1] * Py) + Ef[k, 2] * Pz) + Ef[k, 3]
        return Ef[k, 0] * Px + (Ef[k, 1] * Py + (Ef[k, 2] * Pz + Ef[k, 3]))

    def _integrate_vectorised(self, depth, color, cam, E):
        K = self._frame_constants(depth, cam, E)
        Ef, vl, ul, half = K["Ef"], self.vl, self.ul, 0.5 * self.vl
        U = np.array(self.touched, dtype=np.float64)                       # [n, 3]
        n = len(U)
        g = np.arange(R, dtype=np.float64)
        Px = ((half + vl * g)[None, :, None] + (U[:, 0] * ul)[:, None, None]).astype(f32) + np.zeros((n, R, R), f32)
        Py = ((half + vl * g)[None, None, :] + (U[:, 1] * ul)[:, None, None]).astype(f32) + np.zeros((n, R, R), f32)
        Pz0 = (half + U[:, 2] * ul).astype(f32)[:, None, None] + np.zeros((n, R, R), f32)
        pc = [self._matvec(Ef, k, Px, Py, Pz0) for k in range(3)]
        step = [Ef[k, 2] * K["vlf"] for k in range(3)]
        T = np.stack([self.units[key][0] for key in self.touched])        # [n, x, y, z]
        Wt = np.stack([self.units[key][1] for key in self.touched])
        C = np.stack([self.units[key][2] for key in self.touched]) if self.color else None   # [n, 3, x, y, z]
        with np.errstate(all="ignore"):
            for z in range(R):
                if not QUIRK_TSDF_Z_RUNNING_SUM and z:
                    Pz = (half + vl * z + U[:, 2] * ul).astype(f32)[:, None, None] + np.zeros((n, R, R), f32)
                    pc = [self._matvec(Ef, k, Px, Py, Pz) for k in range(3)]
                m = pc[2] > 0
                uf = (pc[0] * K["fxf"]) / pc[2] + K["cxf"] + f32(0.5)
                vf = (pc[1] * K["fyf"]) / pc[2] + K["cyf"] + f32(0.5)
                m &= (uf >= f32(0.0001)) & (uf < K["wlim"]) & (vf >= f32(0.0001)) & (vf < K["hlim"])
                u, v = np.where(m, uf, 0).astype(np.int32), np.where(m, vf, 0).astype(np.int32)
                d = depth[v, u]
                m &= d > 0
                xx, yy = (u.astype(f32) - K["cxf"]) * K["ifx"], (v.astype(f32) - K["cyf"]) * K["ify"]
                mult = np.sqrt(xx * xx + yy * yy + f32(1))
                sdf = (d - pc[2]) * mult
                m &= sdf > -K["truncf"]
                t = np.minimum(f32(1), sdf * K["itrunc"])
                w0, f0 = Wt[..., z], T[..., z]
                T[..., z] = np.where(m, (f0 * w0 + t) / (w0 + f32(1)), f0)
                if self.color:
                    w64 = w0.astype(np.float64)
                    for ch in range(3):
                        c0 = C[:, ch, :, :, z]
                        C[:, ch, :, :, z] = np.where(m, (c0 * w64 + color[v, u, ch].astype(np.float64)) / (w64 + 1.0), c0)
                Wt[..., z] = np.where(m, w0 + f32(1), w0)
                if QUIRK_TSDF_Z_RUNNING_SUM:
                    pc = [pc[k] + step[k] for k in range(3)]
        for q, key in enumerate(self.touched):
            self.units[key] = [T[q], Wt[q], C[q] if self.color else None]

    def _integrate_literal(self, depth, color, cam, E):
        K = self._frame_constants(depth, cam, E)
        Ef, vl, ul, half = K["Ef"], self.vl, self.ul, 0.5 * self.vl
        for key in self.touched:
            T, Wt, C = self.units[key]
            org = [key[k] * ul for k in range(3)]
            for x in range(R):
                for y in range(R):
                    P = (f32(half + vl * x + org[0]), f32(half + vl * y + org[1]), f32(half + org[2]))
                    pc = [self._matvec(Ef, k, *P) for k in range(3)]
                    for z in range(R):
                        if not QUIRK_TSDF_Z_RUNNING_SUM and z:
                            pc = [self._matvec(Ef, k, P[0], P[1], f32(half + vl * z + org[2])) for k in range(3)]
                        if pc[2] > 0:
                            uf = pc[0] * K["fxf"] / pc[2] + K["cxf"] + f32(0.5)
                            vf = pc[1] * K["fyf"] / pc[2] + K["cyf"] + f32(0.5)
                            if uf >= f32(0.0001) and uf < K["wlim"] and vf >= f32(0.0001) and vf < K["hlim"]:
                                u, v = int(uf), int(vf)
                                d = depth[v, u]
                                if d > 0:
                                    xx, yy = (f32(u) - K["cxf"]) * K["ifx"], (f32(v) - K["cyf"]) * K["ify"]
                                    mult = np.sqrt(xx * xx + yy * yy + f32(1))
                                    sdf = (d - pc[2]) * mult
                                    if sdf > -K["truncf"]:
                                        t = min(f32(1), sdf * K["itrunc"])
                                        w0 = Wt[x, y, z]
                                        T[x, y, z] = (T[x, y, z] * w0 + t) / (w0 + f32(1))
                                        if self.color:
                                            for ch in range(3):
                                                C[ch, x, y, z] = (C[ch, x, y, z] * float(w0) + float(color[v, u, ch])) / (float(w0) + 1.0)
                                        Wt[x, y, z] = w0 + f32(1)
                        if QUIRK_TSDF_Z_RUNNING_SUM:
                            pc = [pc[k] + Ef[k, 2] * K["vlf"] for k in range(3)]

    # ---- state as the debug entry point returns it ----------------------------------------------------------------------------
    def state(self):
        """-> idx int32 [n,3] in (X, Y, Z) order, tsdf f32 [n,4096], weight f32 [n,4096], colour f64 [n,3,4096] (or None)"""
        keys = sorted(self.units)
        n = len(keys)
        idx = np.array(keys, dtype=np.int32).reshape(n, 3)
        T = np.stack([self.units[k][0] for k in keys]).reshape(n, R ** 3) if n else np.zeros((0, R ** 3), f32)
        Wt = np.stack([self.units[k][1] for k in keys]).reshape(n, R ** 3) if n else np.zeros((0, R ** 3), f32)
        C = None
        if self.color:
            C = np.stack([self.units[k][2] for k in keys]).reshape(n, 3, R ** 3) if n else np.zeros((0, 3, R ** 3))
        return idx, T, Wt, C

    # ---- extraction -----------------------------------------------------------------------------------------------------------
    def extract_point_cloud(self, literal=False):
        """-> points, normals, colours (None without colour): float64 [m,3]"""
        if not self.units:
            return np.zeros((0, 3)), np.zeros((0, 3)), (np.zeros((0, 3)) if self.color else None)
        if not QUIRK_TSDF_NORMAL_IGNORES_WEIGHT:
            raise NotImplementedError("only Open3D's weight-blind normal is restated")
        return self._extract_literal() if literal else self._extract_vectorised()

    @staticmethod
    def _usable(w, f):
        return (w != 0) & (f < f32(0.98)) & (f >= f32(-0.98))

    def _extract_vectorised(self):
        keys = sorted(self.units)
        n, vl, ul, half = len(keys), self.vl, self.ul, 0.5 * self.vl
        U = np.array(keys, dtype=np.int64)
        packed = ((U[:, 0] + _LIMIT) << 42) | ((U[:, 1] + _LIMIT) << 21) | (U[:, 2] + _LIMIT)      # ascending with (X, Y, Z)
        T = np.stack([self.units[k][0] for k in keys])
        Wt = np.stack([self.units[k][1] for k in keys])
        C = np.stack([self.units[k][2] for k in keys]) if self.color else None

        def lookup(Ux, Uy, Uz):
            inr = (Ux >= -_LIMIT) & (Ux < _LIMIT) & (Uy >= -_LIMIT) & (Uy < _LIMIT) & (Uz >= -_LIMIT) & (Uz < _LIMIT)
            key = ((Ux + _LIMIT) << 42) | ((Uy + _LIMIT) << 21) | (Uz + _LIMIT)
            pos = np.minimum(np.searchsorted(packed, key), n - 1)
            return np.where(inr & (packed[pos] == key), pos, -1)

        usable0 = self._usable(Wt, T)
        cand = np.zeros((n, R, R, R, 3), bool)
        gx, gy, gz = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
        own = np.arange(n)[:, None, None, None]
        for a in range(3):
            e = np.eye(3, dtype=np.int64)[a]
            nxt = lookup(U[:, 0] + e[0], U[:, 1] + e[1], U[:, 2] + e[2])[:, None, None, None]
            v = [gx + e[0], gy + e[1], gz + e[2]]
            past = v[a] > R - 1
            v[a] = np.where(past, 0, v[a])
            unit = np.where(past[None], nxt, own)
            safe = np.maximum(unit, 0)
            f1, w1 = T[safe, v[0][None], v[1][None], v[2][None]], Wt[safe, v[0][None], v[1][None], v[2][None]]
            cand[..., a] = usable0 & (unit >= 0) & self._usable(w1, f1) & (T * f1 < 0)
        ui, x, y, z, a = np.nonzero(cand)      # row-major: units, then flat voxel index, then axis
        m = len(ui)
        nv = np.stack([x, y, z], 1) + np.eye(3, dtype=np.int64)[a]
        past = nv > R - 1
        nv = np.where(past, 0, nv)
        W = U[ui] + past
        nu = lookup(W[:, 0], W[:, 1], W[:, 2])
        f0, f1 = T[ui, x, y, z], T[nu, nv[:, 0], nv[:, 1], nv[:, 2]]
        r0f, r1f = np.abs(f0), np.abs(f1)
        r0, r1, rs = r0f.astype(np.float64), r1f.astype(np.float64), (r0f + r1f).astype(np.float64)
        p = np.stack([(half + vl * x) + U[ui, 0] * ul, (half + vl * y) + U[ui, 1] * ul, (half + vl * z) + U[ui, 2] * ul], 1)
        rows = np.arange(m)
        pa = p[rows, a]
        p[rows, a] = (pa * r1 + (pa + vl) * r0) / rs
        colours = None
        if self.color:
            c0, c1 = C[ui, :, x, y, z], C[nu, :, nv[:, 0], nv[:, 1], nv[:, 2]]
            colours = ((c0 * r1[:, None] + c1 * r0[:, None]) / rs[:, None]) / 255.0

        def tsdf_at(q):
            ql = q - half
            Uq = np.floor(ql / ul)
            g = (ql - Uq * ul) / vl
            i0 = np.clip(np.floor(g), 0, R - 1)
            r = g - i0
            Uq, i0 = Uq.astype(np.int64), i0.astype(np.int64)
            home = lookup(Uq[:, 0], Uq[:, 1], Uq[:, 2])
            f = []
            for off in _CORNERS:
                v = i0 + np.array(off)
                wrap = v > R - 1
                v = np.where(wrap, 0, v)
                W = Uq + wrap
                s = lookup(W[:, 0], W[:, 1], W[:, 2])
                s = np.where(home >= 0, s, -1)
                f.append(np.where(s >= 0, T[np.maximum(s, 0), v[:, 0], v[:, 1], v[:, 2]], f32(0)).astype(np.float64))
            a_, b_, g_ = 1.0 - r[:, 0], 1.0 - r[:, 1], 1.0 - r[:, 2]
            r0_, r1_, r2_ = r[:, 0], r[:, 1], r[:, 2]
            return a_ * (b_ * (g_ * f[0] + r2_ * f[4]) + r1_ * (g_ * f[3] + r2_ * f[7])) + \
                r0_ * (b_ * (g_ * f[1] + r2_ * f[5]) + r1_ * (g_ * f[2] + r2_ * f[6]))

        d = 0.99 * vl
        grad = np.zeros((m, 3))
        for k in range(3):
            qp, qm = p.copy(), p.copy()
            qp[:, k] = p[:, k] + d
            qm[:, k] = p[:, k] - d
            grad[:, k] = tsdf_at(qp) - tsdf_at(qm)
        length = np.sqrt((grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2])
        with np.errstate(all="ignore"):
            normals = np.where(length[:, None] != 0, grad / length[:, None], grad)
        return p, normals, colours

    # literal: every voxel, every axis, one at a time
    def _voxel(self, key, v):
        """(tsdf, weight, colour or None) of voxel v of unit key, a coordinate past R-1 wrapping into the next unit; None: absent"""
        key, v = list(key), list(v)
        for k in range(3):
            if v[k] > R - 1:
                v[k] = 0
                key[k] += 1
        u = self.units.get(tuple(key))
        if u is None:
            return None
        return u[0][v[0], v[1], v[2]], u[1][v[0], v[1], v[2]], (u[2][:, v[0], v[1], v[2]] if self.color else None)

    def _tsdf_at(self, q):
        vl, ul, half = self.vl, self.ul, 0.5 * self.vl
        ql = [q[k] - half for k in range(3)]
        Uq = [int(np.floor(ql[k] / ul)) for k in range(3)]
        if tuple(Uq) not in self.units:
            return 0.0
        g = [(ql[k] - Uq[k] * ul) / vl for k in range(3)]
        i0 = [min(max(int(np.floor(g[k])), 0), R - 1) for k in range(3)]
        r = [g[k] - i0[k] for k in range(3)]
        f = []
        for off in _CORNERS:
            got = self._voxel(Uq, [i0[k] + off[k] for k in range(3)])
            f.append(0.0 if got is None else float(got[0]))
        return (1 - r[0]) * ((1 - r[1]) * ((1 - r[2]) * f[0] + r[2] * f[4]) + r[1] * ((1 - r[2]) * f[3] + r[2] * f[7])) + \
            r[0] * ((1 - r[1]) * ((1 - r[2]) * f[1] + r[2] * f[5]) + r[1] * ((1 - r[2]) * f[2] + r[2] * f[6]))

    def _extract_literal(self):
        vl, ul, half = self.vl, self.ul, 0.5 * self.vl
        pts, nrm, col = [], [], []
        for key in sorted(self.units):
            T, Wt, C = self.units[key]
            for x in range(R):
                for y in range(R):
                    for z in range(R):
                        f0, w0 = T[x, y, z], Wt[x, y, z]
                        if not self._usable(w0, f0):
                            continue
                        p0 = [half + vl * x + key[0] * ul, half + vl * y + key[1] * ul, half + vl * z + key[2] * ul]
                        for a in range(3):
                            v = [x, y, z]
                            v[a] += 1
                            got = self._voxel(key, v)
                            if got is None:
                                continue
                            f1, w1, c1 = got
                            if not (self._usable(w1, f1) and f0 * f1 < 0):
                                continue
                            r0f, r1f = abs(f0), abs(f1)
                            r0, r1, rs = float(r0f), float(r1f), float(r0f + r1f)
                            p = list(p0)
                            p[a] = (p0[a] * r1 + (p0[a] + vl) * r0) / rs
                            pts.append(p)
                            if self.color:
                                col.append([((float(C[ch, x, y, z]) * r1 + float(c1[ch]) * r0) / rs) / 255.0 for ch in range(3)])
                            g = []
                            for k in range(3):
                                qp, qm = list(p), list(p)
                                qp[k] = p[k] + 0.99 * vl
                                qm[k] = p[k] - 0.99 * vl
                                g.append(self._tsdf_at(qp) - self._tsdf_at(qm))
                            length = float(np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
                            nrm.append([gk / length for gk in g] if length != 0 else g)
        return (np.array(pts, dtype=np.float64).reshape(-1, 3), np.array(nrm, dtype=np.float64).reshape(-1, 3),
                np.array(col, dtype=np.float64).reshape(-1, 3) if self.color else None)


def poses_from_edges(edges):
    """camera-to-world poses along a chain, the first frame the world.  An edge (source k+1 -> target k, T) says x_k = T x_k+1,
    so pose_k+1 = pose_k T; an edge (source k -> target k+1, T), the direction of test/check84.py's loop, says x_k+1 = T x_k,
    so pose_k+1 = pose_k inv(T) -- which is that loop's inv(T_n .. T_1)."""
    poses = [np.eye(4)]
    for k, e in enumerate(edges):
        T = np.asarray(e["T"], dtype=np.float64)
        poses.append(poses[-1] @ (T if (e["source"], e["target"]) == (k + 1, k) else np.linalg.inv(T)))
    return poses
