"""NumPy twin of csrc/selflow_aug.hip (fn2_selflow_stats + fn2_selflow_apply) for the tests: integer-exact for the
hash, the masks and everything that only moves data, float64 for the colour arithmetic.  It restates the definitions in
include/flownet2_hip.h; it shares no code with src/data_augmentation.py except the word offsets of the record."""
import numpy as np

(DISTRIB, THRESHOLD, KEY0, KEY1, N_RECT, RECTS, FLIP_LR, FLIP_UD, PERM, COLOUR_ORDER, D_BRIGHTNESS, F_SATURATION, D_HUE,
 F_CONTRAST) = 0, 1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 22, 23, 24
PARAM_WORDS = 32
FMIX_C1, FMIX_C2 = 0x85EBCA6B, 0xC2B2AE35
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
# op codes: B brightness, S saturation, H hue, C contrast
CHAINS = ("BSHC", "SBCH", "CHBS", "HSCB")
HAZARD_EPS = 1e-6


def fmix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(FMIX_C1)
    x ^= x >> np.uint32(13)
    x *= np.uint32(FMIX_C2)
    x ^= x >> np.uint32(16)
    return x


def hash_u(i, key0, key1):
    """u(i) = fmix32(fmix32(i ^ key0) + key1), uint32 arithmetic."""
    i = np.asarray(i, np.uint32)
    return fmix32(fmix32(i ^ np.uint32(key0)) + np.uint32(key1))


def uniform_mask(h, w, threshold, key0, key1):
    i = np.arange(h * w, dtype=np.uint32).reshape(h, w)
    return hash_u(i, key0, key1) < np.uint32(threshold)


def threshold_of(p):
    """min(floor(p * 2^32), 2^32 - 1) for a float32 p, in exact integer arithmetic."""
    num, den = float(np.float32(p)).as_integer_ratio()
    return int(min(max((num << 32) // den, 0), (1 << 32) - 1))


def resampled_mask(rec, h, w):
    """The mask of distrib 1 / 2 in source coordinates (bool [h, w])."""
    if int(rec[DISTRIB]) == 1:
        return uniform_mask(h, w, rec[THRESHOLD], rec[KEY0], rec[KEY1])
    m = np.ones((h, w), bool)
    r = rec.view(np.int32)
    for k in range(min(max(int(r[N_RECT]), 0), 3)):
        y0, x0, rh, rw = (int(v) for v in r[RECTS + 4 * k:RECTS + 4 * k + 4])
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        m &= ~((ys >= y0) & (ys < y0 + rh) & (xs >= x0) & (xs < x0 + rw))
    return m


def keeps_resampled(count, hw):
    """sample_from_distribution's test in float32: 100 * (count / hw) >= 0.01."""
    return bool(np.float32(100.0) * (np.float32(count) / np.float32(hw)) >= np.float32(0.01))


def rgb_to_hsv(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = rgb.max(-1)
    rng = v - rgb.min(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, rng / v, 0.0)
        h = np.where(r == v, (g - b) / (6 * rng), np.where(g == v, (b - r) / (6 * rng) + 2 / 6, (r - g) / (6 * rng) + 4 / 6))
    h = np.where(rng <= 0, 0.0, h)
    h = np.where(h < 0, h + 1, h)
    return h, s, v


def hsv_to_rgb(h, s, v):
    c = s * v
    m = v - c
    dh = 6 * h
    x = c * (1 - np.abs(np.fmod(dh, 2) - 1))
    k = dh.astype(np.int64)
    k = np.where((k < 0) | (k > 5), 0, k)  # dh == 6 is case 0
    z = np.zeros_like(c)
    table = ((c, x, z), (x, c, z), (z, c, x), (z, x, c), (x, z, c), (c, z, x))
    out = np.stack([np.choose(k, [t[ch] for t in table]) for ch in range(3)], -1)
    return out + m[..., None]


def colour_chain(img, rec):
    """One sample [h, w, 3] (already permuted) through the chain of its record in float64, clipped at the end.
    Returns (image, hazards): hazards = pixels whose max channel lay within HAZARD_EPS of 0 on entry to an HSV op."""
    order = int(rec.view(np.int32)[COLOUR_ORDER])
    x = img.astype(np.float64)
    hazards = np.zeros(x.shape[:2], bool)
    if not 0 <= order <= 3:
        return x, hazards
    f = rec.view(np.float32).astype(np.float64)
    for op in CHAINS[order]:
        if op == "B":
            x = x + f[D_BRIGHTNESS]
        elif op == "C":
            mean = x.mean(axis=(0, 1))
            x = (x - mean) * f[F_CONTRAST] + mean
        else:
            hazards |= np.abs(x.max(-1)) <= HAZARD_EPS
            h, s, v = rgb_to_hsv(x)
            if op == "S":
                s = np.clip(s * f[F_SATURATION], 0.0, 1.0)
            else:
                h = h + f[D_HUE]
                h = h - np.floor(h)
            x = hsv_to_rgb(h, s, v)
    return np.clip(x, 0.0, 1.0), hazards


def apply(params, params_b=None, image_a=None, image_b=None, matches=None, sparse_flow=None, edges=None, flow=None):
    """What fn2_selflow_stats + fn2_selflow_apply compute: dict of outputs (images float64 where a colour chain ran,
    everything else in the input dtype, bit-exact) + 'hazards' (bool [n, h, w])."""
    first = next(t for t in (image_a, image_b, matches, sparse_flow, edges, flow) if t is not None)
    n, h, w = first.shape[:3]
    out = {k: [] for k in ("image_a", "image_b", "matches", "sparse_flow", "edges", "flow", "hazards")}

    for s in range(n):
        rec = params[s]
        lr, ud = bool(rec[FLIP_LR]), bool(rec[FLIP_UD])

        def flip(a):
            a = a[:, ::-1] if lr else a
            return a[::-1] if ud else a

        def flip_flow(a):
            a = flip(a).copy()
            if lr:
                a[..., 0] = -a[..., 0]
            if ud:
                a[..., 1] = -a[..., 1]
            return a

        m_out = None if matches is None else matches[s]
        sf_out = None if sparse_flow is None else sparse_flow[s]
        if int(rec[DISTRIB]) in (1, 2) and flow is not None:
            mask = resampled_mask(rec, h, w)
            if keeps_resampled(int(mask.sum()), h * w):
                m_out = mask.astype(np.float32)[..., None]
                sf_out = np.where(mask[..., None], flow[s], np.float32(0.0)).astype(np.float32)
        if matches is not None:
            out["matches"].append(flip(m_out))
        if sparse_flow is not None:
            out["sparse_flow"].append(flip_flow(sf_out))
        if edges is not None:
            out["edges"].append(flip(edges[s]))
        if flow is not None:
            out["flow"].append(flip_flow(flow[s]))
        hz = np.zeros((h, w), bool)
        for name, img, crec in (("image_a", image_a, rec), ("image_b", image_b, None if params_b is None else params_b[s])):
            if img is None:
                continue
            x = img[s][..., list(PERMS[int(rec[PERM])] if 0 <= int(rec[PERM]) <= 5 else PERMS[0])]
            if 0 <= int(crec.view(np.int32)[COLOUR_ORDER]) <= 3:
                x, hz_i = colour_chain(x, crec)
                hz |= hz_i
            out[name].append(flip(x))
        out["hazards"].append(flip(hz))
    return {k: (np.stack(v) if v else None) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ shared cases
def empty_params(n):
    t = np.zeros((n, PARAM_WORDS), np.uint32)
    t.view(np.int32)[:, COLOUR_ORDER] = -1
    return t


def set_colour(rec, order, d_brightness, f_saturation, d_hue, f_contrast):
    rec.view(np.int32)[COLOUR_ORDER] = order
    rec.view(np.float32)[[D_BRIGHTNESS, F_SATURATION, D_HUE, F_CONTRAST]] = (d_brightness, f_saturation, d_hue, f_contrast)


COLOUR_SHAPES = ((4, 6, 70), (2, 64, 96))
COLOUR_SEEDS = {(4, 6, 70): 101, (2, 64, 96): 202}
# (d_brightness, f_saturation, d_hue, f_contrast) of chain order k: values that clip at both ends, and d_hue exactly 0.5
# on the chain that starts with the hue op (a cyan pixel, h = 0.5, lands on h + d = 1)
COLOUR_SETTINGS = ((0.2, 1.5, 0.1, 1.4), (-0.2, 0.5, -0.2, 0.2), (-0.15, 1.3, 0.2, 1.4), (0.1, 0.7, 0.5, 0.9))
SPECIAL_PIXELS = ((0.5, 0.5, 0.5), (0.2, 0.2, 0.2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1))


def colour_cases():
    """[(name, images float32 [n, h, w, 3], table)] of the GPU colour test: every chain order at both shapes (the 2-sample
    shape in two calls), grey pixels, primaries, cyan, an image with a large constant offset, and black pixels in the
    samples whose chain does not start with an HSV op (an exactly black pixel entering an HSV op has max channel 0, which
    the exclusion check counts)."""
    cases = []
    for shape in COLOUR_SHAPES:
        n, h, w = shape
        rng = np.random.default_rng(COLOUR_SEEDS[shape])
        for first in range(0, 4, n):
            img = rng.random((n, h, w, 3), dtype=np.float32)
            table = empty_params(n)
            for s in range(n):
                order = first + s
                if order == 1:
                    img[s] = np.float32(0.75) + np.float32(0.25) * img[s]  # a wrong mean shows
                flat = img[s].reshape(-1, 3)
                pix = list(SPECIAL_PIXELS) + ([(0, 0, 0)] if order in (0, 2) else [])
                where = rng.choice(h * w, size=2 * len(pix), replace=False)
                flat[where] = np.asarray(pix + pix, np.float32)
                set_colour(table[s], order, *COLOUR_SETTINGS[order])
                table[s, PERM] = (order + 1) % 6
            cases.append(("%dx%dx%d_orders%d-%d" % (n, h, w, first, first + n - 1), img, table))
    return cases
