"""Restatement of StereoSGBM on 3-channel pairs (OpenCV 4.x calcPixelCostBT with cn == 3, [recalled] like SURVEY.md Appendix A).

The pixel cost of a colour pair is the sum over the channels of what the grey routine computes on that channel's plane alone
(Sobel-x prefilter with the grey border rules, BT on the prefiltered values + BT on the raw values >> 2, the shift per channel
before the sum).  The box sum is linear, so the block cost is the sum over the planes of oracle.sgbm_oracle.cost_rows; everything
after the block cost is the grey algorithm:
  * compute_hh: tests.sgbm_hh_ref's aggregate / select / finish on the summed volume;
  * compute_3way: MODE_SGBM_3WAY from the cost volume: four stripes of ceil(H/4) rows, each with overlap warm-up rows above it and
    its block cost replicated at its own first row; L_left, L_right and L_top start at 0, every step saturates to int16,
    S = sat16(L_left + L_right + L_top), then the selection of sgbm_hh_ref.  Images so small that a stripe's warm-up start is
    clamped to row 0 (QUIRK_SMALL_IMAGE_STRIPES of oracle/sgbm3way.c) are refused: that quirk is not restated here.
Grey [H,W] inputs are the one-plane case (the CPU tests pin compute_3way to the C oracle with them).  No product code.
"""
import numpy as np

from tests import sgbm_hh_ref as hh


def color_pair(synth, W, H, D, seed):
    """Colour frames over a textured stereo pair: the grey pair scaled by 0.8 / 1.0 / 0.9 per channel plus 0..11 of noise."""
    L, R, _ = synth.stereo_pair(W, H, D, seed=seed)
    rng = np.random.default_rng(seed)

    def colour(g):
        f = g.astype(np.float64)[:, :, None] * np.array([0.8, 1.0, 0.9]) + rng.integers(0, 12, g.shape + (3,))
        return np.clip(f, 0, 255).astype(np.uint8)
    return colour(L), colour(R)


def _planes(a):
    a = np.asarray(a)
    return [a] if a.ndim == 2 else [np.ascontiguousarray(a[:, :, c]) for c in range(a.shape[2])]


def block_cost(L, R, kw, band_start, y0, y1):
    """C[y - y0][xc][d] (int32) of rows [y0, y1) of a stripe whose first row is band_start: the sum over the planes."""
    from oracle import sgbm_oracle as so
    p = so.make_params(**kw)
    return sum(so.cost_rows(l, r, p, band_start, y0, y1).astype(np.int32) for l, r in zip(_planes(L), _planes(R)))


def _finish(raw, g, return_raw):
    out = hh.finish(raw, g)
    return (out, raw) if return_raw else out


def compute_hh(L, R, return_raw=False, **kw):
    H, W = np.asarray(L).shape[:2]
    g = hh.derive(W, **kw)
    assert g["W1"] > 0
    S = hh.aggregate(block_cost(L, R, kw, 0, 0, H), g["P1"], g["P2"])
    return _finish(hh.select(S, g, W), g, return_raw)


def _rows_scan(C, P1, P2, xs):
    """One horizontal path over every row at once: int32 [H, W1, D]."""
    H, W1, D = C.shape
    out = np.empty(C.shape, np.int32)
    Lp, mp = np.zeros((H, D), np.int32), np.zeros(H, np.int32)
    for x in xs:
        Lp, _ = hh._step(C[:, x], Lp, mp, P1, P2)
        Lp = hh._sat16(Lp)
        mp = Lp.min(axis=1)
        out[:, x] = Lp
    return out


def stripe_sums(L, R, return_cost=False, **kw):
    """S (int16 [H, W1, D]) of MODE_SGBM_3WAY, every row taken from the stripe that owns it."""
    H, W = np.asarray(L).shape[:2]
    g = hh.derive(W, **kw)
    assert g["W1"] > 0
    P1, P2, bs = g["P1"], g["P2"], kw.get("blockSize", 3)
    ss = (H + 3) // 4
    overlap = bs // 2 + 1 + (ss + 9) // 10
    S = np.empty((H, g["W1"], g["D"]), np.int16)
    for n in range(4):
        own0, y1 = n * ss, min((n + 1) * ss, H)
        if own0 >= y1:
            continue
        assert n == 0 or own0 - overlap >= 0, "tiny-image stripe quirk: not restated here"
        y0 = max(own0 - overlap, 0)
        C = block_cost(L, R, kw, y0, y0, y1)
        Lh = _rows_scan(C, P1, P2, range(g["W1"])) + _rows_scan(C, P1, P2, range(g["W1"] - 1, -1, -1))
        Lp, mp = np.zeros((g["W1"], g["D"]), np.int32), np.zeros(g["W1"], np.int32)
        for y in range(y0, y1):
            Lp, _ = hh._step(C[y - y0], Lp, mp, P1, P2)
            Lp = hh._sat16(Lp)
            mp = Lp.min(axis=1)
            if y >= own0:
                S[y] = hh._sat16(Lh[y - y0] + Lp)
    return S


def compute_3way(L, R, return_raw=False, **kw):
    H, W = np.asarray(L).shape[:2]
    g = hh.derive(W, **kw)
    return _finish(hh.select(stripe_sums(L, R, **kw), g, W), g, return_raw)
