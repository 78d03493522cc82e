"""Generate tests/golden/variational_edges_golden.npz by RUNNING the reference's EpicFlow variational refinement
(src/SrcVariational) on the regimes variational_golden.npz never reaches (build container only: needs
/root/reference and gcc).  variational_golden.npz is neither read for writing nor regenerated here.

The driver, the PPM / .flo helpers and init_from are those of make_golden_variational.py.  The driver is built
twice in a temporary directory, `gcc -O3 -msse4` as the reference's Makefile builds its binary, and the same with
`-fsanitize=address` (run with ASAN_OPTIONS=detect_leaks=0: the driver never frees its images).  A case is stored
only if the sanitizer build exits clean and writes the same bits as the plain build.

Frames and ground truth are the committed samples (0img0.ppm -> 0img1.ppm, 0flow.flo), not stored again:
  crop frames   rows y0.., columns x0.. of the samples with (y0, x0) = ORIGIN, cut to the case's size
  tall frames   the 12-column strips at x = 100, 250, 400 of each sample, stacked vertically (1152x12), cut to the
                case's height; the ground truth is stacked the same way
Inits are ground truth + q / 2 with a seeded int8 q per image size (`q_<H>x<W>`, N(0, 0.75 px) in half pixels);
`far` adds `far_off`, a seeded choice of {-60, 0, 0, +60} half pixels per component (+-30 px).  case_inputs() below
builds every input from the samples and those arrays; the GPU tests call it too, so the two cannot drift.  No random
numbers are drawn at test time.

Per case the file holds `<name>_out` (the reference's output on the FULL pixel grid), `<name>_params` and
`<name>_spread`: the reference is run twice more with every init component moved one float32 ulp up, and one ulp
down, and the spread is (mean, p99.9, max) of the end-point distance to the un-nudged output, the larger of the two
runs for each statistic.  `crop_spread` is the same measurement for the `crop` case of variational_golden.npz (its
init rebuilt from that file's `crop_q`).  The tests scale the project's EPE tolerances by spread(case) /
spread(crop), so no bound comes from the GPU code.  A case whose spread maximum exceeds SPREAD_CAP is too badly
conditioned to pin anything and is refused.

One thing makes the reference jump under such a nudge: an init that points EXACTLY at the first row or column of
the frame (x + u == 0), where image_warp's in-image mask switches off one ulp further out.  The samples' ground truth
is a multiple of 1/32 px and q of 1/2 px, so this happens: off_the_border() moves q one step at such components
(and at the last row / column, for symmetry).  The `crop` init has two such pixels, which its crop_q fixes: its
downward run moves by up to 0.84 px (upward: 4.7e-4 px), `crop_spread` records that as measured and is not held to
the cap, and with it every ratio spread(case) / spread(crop) is below 1: the new cases are held to the project's
tolerances unscaled, and their maximum to the p99.9 tolerance.

Moving every init off the border leaves the mask's own edge unpinned: with `<` for `<=` in image_warp all twenty
cases above give the same bits.  `far_edge` closes that: `far`'s init at one outer iteration, with the ten pixels of
EDGE_PINS set to point exactly at the last column, the first column, the last row and the first row (case_inputs).
There i + u is an exact integer in float32 for the reference and for var_warp alike, so the comparison is
deterministic; the one-ulp spread of this case nudges every pixel but the pinned ones.

Cases with sigma <= 0.66 keep niter_outer = 1 (with two outer iterations at sigma 0.3 the reference's own answer
moves by pixels under a one-ulp nudge); `col` is the exception the spread cap allows.  The reference reads out of
bounds when a dimension is below 2 * order + 1 with order >= 3, or when h <= 3: no such case is here.

The archive is written with fixed member timestamps, so a rerun reproduces the committed file byte for byte.

    python tests/golden/make_golden_variational_edges.py
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from make_golden_variational import (CROP, DEFAULTS, DRIVER, REF, SAMPLES, init_from, read_flo,  # noqa: E402
                                     read_ppm, write_flo, write_ppm)

FIXTURE = "variational_edges_golden.npz"
ORIGIN = (100, 130)            # y0, x0 of every crop
STRIP_X, STRIP_W = (100, 250, 400), 12
SEED = 20261018
SPREAD_CAP = 1e-3              # px: the largest one-ulp spread maximum a stored case may have
PARAM_KEYS = ("alpha", "gamma", "delta", "sigma", "niter_outer", "niter_inner", "niter_solver", "sor_omega")

# name, (H, W), frames ("crop" | "tall"), parameters that differ from the defaults
CASES = [
    ("delta", (48, 64), "crop", dict(delta=0.5, niter_outer=2)),
    ("delta_only", (48, 64), "crop", dict(delta=1.0, gamma=0.0, niter_outer=2)),
    ("inner2", (48, 64), "crop", dict(niter_inner=2, niter_outer=2, niter_solver=10)),
    ("inner3", (48, 64), "crop", dict(niter_inner=3, niter_outer=1, niter_solver=5)),
    ("sig03", (48, 64), "crop", dict(sigma=0.3, niter_outer=1)),
    ("sig066", (48, 64), "crop", dict(sigma=0.66, niter_outer=1)),
    ("sig3", (48, 64), "crop", dict(sigma=3.0, niter_outer=2)),
    ("sig10", (63, 63), "crop", dict(sigma=10.0, niter_outer=2)),
    ("min9", (9, 9), "crop", dict(niter_outer=2)),
    ("w2", (33, 2), "crop", dict(sigma=0.3, niter_outer=1)),
    ("w3", (33, 3), "crop", dict(sigma=0.3, niter_outer=1)),
    ("w4", (33, 4), "crop", dict(sigma=0.5, niter_outer=1)),
    ("h4", (4, 33), "crop", dict(sigma=0.5, niter_outer=1)),
    ("h5", (5, 33), "crop", dict(sigma=0.5, niter_outer=1)),
    ("col", (40, 1), "crop", dict(sigma=0.3, niter_outer=2, niter_solver=10)),
    ("h600", (600, 12), "tall", dict(niter_outer=2)),
    ("tall", (1100, 12), "tall", dict(niter_outer=2)),
    ("far", (48, 64), "crop", dict(niter_outer=2)),
    ("omega1", (48, 64), "crop", dict(sor_omega=1.0, niter_outer=2)),
    ("alpha3", (48, 64), "crop", dict(alpha=3.0, niter_outer=2)),
    ("far_edge", (48, 64), "crop", dict(niter_outer=1)),
]
# far_edge: (row j, column i, side) of the pixels whose init points EXACTLY at a border row / column of the frame
EDGE_PINS = [(10, 20, "right"), (30, 50, "right"), (21, 3, "right"), (44, 33, "right"), (12, 40, "left"),
             (35, 10, "left"), (20, 15, "bottom"), (5, 45, "bottom"), (40, 30, "top"), (25, 60, "top")]
CASE_NAMES = [c[0] for c in CASES]
_BY_NAME = {c[0]: c for c in CASES}


def load_samples(samples_dir=SAMPLES):
    """The committed pair and its ground truth: uint8 [384, 512, 3] x2, float32 [384, 512, 2]."""
    a = read_ppm(os.path.join(samples_dir, "0img0.ppm"))
    b = read_ppm(os.path.join(samples_dir, "0img1.ppm"))
    gt = read_flo(os.path.join(samples_dir, "0flow.flo")).astype(np.float32)
    return a, b, gt


def cut(x, shape, frames):
    """The [H, W] cut of a sample array `x` ([384, 512, C]) that the cases of kind `frames` run on."""
    h, w = shape
    if frames == "tall":
        assert w == STRIP_W
        return np.ascontiguousarray(np.concatenate([x[:, s:s + STRIP_W] for s in STRIP_X], 0)[:h])
    y0, x0 = ORIGIN
    out = np.ascontiguousarray(x[y0:y0 + h, x0:x0 + w])
    assert out.shape[:2] == (h, w)
    return out


def q_key(shape):
    return "q_%dx%d" % tuple(shape)


def case_params(name):
    return dict(DEFAULTS, **_BY_NAME[name][3])


def case_inputs(name, samples, arrays):
    """(img_a, img_b, init, params) of case `name`: `samples` from load_samples(), `arrays` a mapping that holds
    the int8 perturbations `q_<H>x<W>` and `far_off` (the fixture, or the generator's fresh draws)."""
    _, shape, frames, _ = _BY_NAME[name]
    a, b, gt = (cut(x, shape, frames) for x in samples)
    q = np.asarray(arrays[q_key(shape)]).astype(np.int16)
    if name in ("far", "far_edge"):
        q = q + np.asarray(arrays["far_off"]).astype(np.int16)
    init = init_from(gt, q)
    if name == "far_edge":
        init[edge_pins(shape)] = edge_values(shape)
    return a, b, init, case_params(name)


def edge_pins(shape):
    """Boolean [H, W] mask of far_edge's pinned pixels."""
    m = np.zeros(shape, bool)
    for j, i, _ in EDGE_PINS:
        m[j, i] = True
    return m


def edge_values(shape):
    """The inits of far_edge's pinned pixels, in row-major pixel order: one component lands exactly on the first
    or last column / row (integers: i + u is exact in float32, here and in the reference), the other stays a
    quarter pixel inside the frame, so the in-image mask of each pinned pixel is decided by the `<=` alone."""
    h, w = shape
    val = {"right": lambda j, i: (w - 1 - i, 0.25), "left": lambda j, i: (-i, 0.25),
           "bottom": lambda j, i: (0.25, h - 1 - j), "top": lambda j, i: (0.25, -j)}
    return np.array([val[side](j, i) for j, i, side in sorted(EDGE_PINS)], np.float32)


def epe_stats(got, want):
    """mean, p99.9 and max of the end-point distance, in float64."""
    e = np.sqrt(((np.asarray(got, np.float64) - np.asarray(want, np.float64)) ** 2).sum(-1))
    return float(e.mean()), float(np.percentile(e, 99.9)), float(e.max())


def off_the_border(gt, q):
    """q (int16, half pixels) moved by one step wherever ground truth + q / 2 points EXACTLY at the first or last
    row or column of the frame.  image_warp's in-image mask (0 <= x <= w - 1, 0 <= y <= h - 1) switches there, so
    the reference's own answer jumps when such an init moves by one ulp; no perturbation may sit on that edge."""
    h, w = gt.shape[:2]
    jj, ii = np.mgrid[0:h, 0:w].astype(np.float32)
    q = q.copy()
    for _ in range(4):
        init = init_from(gt, q)
        xx, yy = ii + init[..., 0], jj + init[..., 1]
        hit = np.stack([(xx == 0) | (xx == w - 1), (yy == 0) | (yy == h - 1)], -1)
        if not hit.any():
            return q
        q[hit] += np.where(q[hit] > 0, -1, 1)
    raise AssertionError("perturbation still points at the frame's border")


def draw_arrays(rng, samples):
    """The seeded perturbations: one q per image size in table order, then far's offsets."""
    arrays = {}
    for _, shape, frames, _ in CASES:
        if q_key(shape) not in arrays:  # N(0, 0.75 px) in half pixels
            q = np.clip(np.round(rng.normal(0.0, 0.75, shape + (2,)) * 2), -60, 60).astype(np.int16)
            arrays[q_key(shape)] = off_the_border(cut(samples[2], shape, frames), q).astype(np.int8)
    _, shape, frames, _ = _BY_NAME["far"]
    q = arrays[q_key(shape)].astype(np.int16)
    off = rng.choice(np.array([-60, 0, 0, 60], np.int16), shape + (2,))
    arrays["far_off"] = (off_the_border(cut(samples[2], shape, frames), q + off) - q).astype(np.int8)
    return arrays


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (the archive's bytes then depend on its contents alone)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


class Reference:
    """The reference driver, plain and under AddressSanitizer, in a temporary directory."""

    def __init__(self, tmp):
        self.tmp = tmp
        src = os.path.join(tmp, "driver.c")
        with open(src, "w") as f:
            f.write(DRIVER)
        sources = [os.path.join(REF, s) for s in ("variational.c", "variational_aux.c", "solver.c", "image.c")]
        self.exe, self.exe_asan = os.path.join(tmp, "variational_driver"), os.path.join(tmp, "variational_driver_asan")
        base = ["gcc", "-O3", "-msse4", "-I", REF, src] + sources
        subprocess.run(base + ["-lm", "-o", self.exe], check=True)
        subprocess.run(base + ["-g", "-fsanitize=address", "-lm", "-o", self.exe_asan], check=True)

    def run(self, tag, a, b, init, p, sanitize=False):
        pa, pb = os.path.join(self.tmp, tag + "_a.ppm"), os.path.join(self.tmp, tag + "_b.ppm")
        fi, fo = os.path.join(self.tmp, tag + "_in.flo"), os.path.join(self.tmp, tag + "_out.flo")
        write_ppm(pa, a)
        write_ppm(pb, b)
        write_flo(fi, init)
        args = [repr(float(np.float32(p[k]))) for k in ("alpha", "gamma", "delta", "sigma")]
        args += [str(p[k]) for k in ("niter_outer", "niter_inner", "niter_solver")]
        args += [repr(float(np.float32(p["sor_omega"])))]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        subprocess.run([self.exe_asan if sanitize else self.exe, pa, pb, fi, fo] + args, check=True, env=env)
        res = read_flo(fo)
        assert res.shape == init.shape and np.isfinite(res).all(), tag
        return res

    def case(self, name, a, b, init, p, cap=SPREAD_CAP, hold=None):
        """(output, spread) of one case; raises unless the sanitizer build is clean and gives the same bits, and the
        spread maximum is within `cap`.  Pixels of the boolean [H, W] mask `hold` are not nudged."""
        out = self.run(name, a, b, init, p)
        san = self.run(name + "_asan", a, b, init, p, sanitize=True)
        assert out.tobytes() == san.tobytes(), "%s: sanitizer build differs from the plain build" % name
        keep = np.zeros(init.shape[:2], bool) if hold is None else hold
        up = self.run(name + "_up", a, b, np.where(keep[..., None], init, np.nextafter(init, np.float32(np.inf))), p)
        dn = self.run(name + "_dn", a, b, np.where(keep[..., None], init, np.nextafter(init, np.float32(-np.inf))), p)
        spread = np.maximum(epe_stats(up, out), epe_stats(dn, out))
        assert spread[2] <= cap, "%s: one-ulp spread max %.2e px > cap %.0e" % (name, spread[2], cap)
        return out, spread


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference sources at %s" % REF)
    samples = load_samples()
    arrays = draw_arrays(np.random.default_rng(SEED), samples)
    out = {"cases": np.array(CASE_NAMES), "shapes": np.array([c[1] for c in CASES]), "origin": np.array(ORIGIN)}
    out.update(arrays)
    with tempfile.TemporaryDirectory() as tmp:
        ref = Reference(tmp)
        # the yardstick: the `crop` case of variational_golden.npz, its init rebuilt from that file's crop_q
        with np.load(os.path.join(HERE, "variational_golden.npz")) as z:
            crop_q, crop_out, step = z["crop_q"], z["crop_out"], int(z["grid_step"])
        y0, x0, ch, cw = CROP
        ca, cb, cgt = (np.ascontiguousarray(x[y0:y0 + ch, x0:x0 + cw]) for x in samples)
        res, spread = ref.case("crop", ca, cb, init_from(cgt, crop_q), DEFAULTS, cap=np.inf)
        rows, cols = np.unique(np.r_[np.arange(0, ch, step), ch - 1]), np.unique(np.r_[np.arange(0, cw, step), cw - 1])
        assert np.array_equal(res[rows][:, cols], crop_out), "crop: not the bits of variational_golden.npz"
        out["crop_spread"] = spread
        print("%-11s %4dx%-3d spread mean %.1e  p99.9 %.1e  max %.1e px" % (("crop", ch, cw) + tuple(spread)))
        for name, shape, _, _ in CASES:
            a, b, init, p = case_inputs(name, samples, arrays)
            res, spread = ref.case(name, a, b, init, p, hold=edge_pins(shape) if name == "far_edge" else None)
            out[name + "_out"] = res
            out[name + "_params"] = np.array([p[k] for k in PARAM_KEYS], np.float64)
            out[name + "_spread"] = spread
            print("%-11s %4dx%-3d spread mean %.1e  p99.9 %.1e  max %.1e px   mean |out - init| = %.4f px"
                  % ((name,) + shape + tuple(spread) + (float(np.abs(res - init).mean()),)))
    dst = os.path.join(HERE, FIXTURE)
    save_npz(dst, out)
    print("wrote %s (%.2f MB)" % (dst, os.path.getsize(dst) / 1e6))


if __name__ == "__main__":
    main()
