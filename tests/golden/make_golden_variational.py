"""Generate tests/golden/variational_golden.npz by RUNNING the reference's EpicFlow variational refinement
(src/SrcVariational: variational.c, variational_aux.c, solver.c, image.c) on the committed sample pair
(build container only: needs /root/reference and gcc).

The reference's own main (variational_main.cpp) decodes images through io.c, which needs libjpeg / libpng headers;
instead a small driver written here reads binary PPM and Middlebury .flo files, fills the reference's image
structures and calls its variational() with explicit parameters.  It is compiled in a temporary directory with
`gcc -O3 -msse4 -lm`, as the reference's Makefile builds the binary.

The file stays small (about 0.5 MB): the frames and the ground truth are the committed samples (not stored again);
the perturbed inits are stored as their int8 perturbation in half pixels (init = ground truth + q / 2, exact in
float32), the network-like init as fp16 (it holds fp16 values); the reference's outputs are stored on the pixel
grid `sample_grid` (every 4th row and column plus the last row and column), where the tests compare.  No random
numbers are drawn at test time.

Cases (all on samples/0img0.ppm -> 0img1.ppm, ground truth samples/0flow.flo):
  full        512x384, init = ground truth + seeded perturbation, default parameters
  crop        254x190 crop (width % 4 != 0; adapt_x_u8 pads it to 256x192), same kind of init, defaults
  crop_net    the crop, init = ground truth box-downsampled x4 and upsampled (network-like), defaults
  crop_o1s1   crop with niter_outer=1, niter_solver=1   (pins the system build)
  crop_o1s30  crop with niter_outer=1, niter_solver=30  (pins one full solve)
  crop_kitti  crop with the -kitti preset

    python tests/golden/make_golden_variational.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference/src/SrcVariational"
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, "samples")
CROP = (100, 130, 190, 254)  # y0, x0, h, w
GRID_STEP = 4

# variational_params_default (variational.c:85-98) and the presets of variational_main.cpp:63-84
DEFAULTS = dict(alpha=1.0, gamma=0.71, delta=0.0, sigma=1.0, niter_outer=5, niter_inner=1, niter_solver=30,
                sor_omega=1.9)
KITTI = dict(DEFAULTS, niter_outer=2, alpha=1.0, gamma=0.77, delta=0.0, sigma=1.7)

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "image.h"
#include "variational.h"

static color_image_t *read_ppm(const char *path) {
    FILE *f = fopen(path, "rb");
    int w, h, maxv;
    if (!f || fscanf(f, "P6 %d %d %d", &w, &h, &maxv) != 3 || maxv != 255) { fprintf(stderr, "bad ppm %s\n", path); exit(2); }
    fgetc(f);
    unsigned char *buf = malloc((size_t)w * h * 3);
    if (fread(buf, 1, (size_t)w * h * 3, f) != (size_t)w * h * 3) { fprintf(stderr, "short ppm %s\n", path); exit(2); }
    fclose(f);
    color_image_t *im = color_image_new(w, h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const unsigned char *p = buf + ((size_t)y * w + x) * 3;
            im->c1[y * im->stride + x] = p[0];
            im->c2[y * im->stride + x] = p[1];
            im->c3[y * im->stride + x] = p[2];
        }
    free(buf);
    return im;
}

static void read_flo(const char *path, image_t **wx, image_t **wy) {
    FILE *f = fopen(path, "rb");
    float tag; int w, h;
    if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1) { fprintf(stderr, "bad flo\n"); exit(2); }
    *wx = image_new(w, h); *wy = image_new(w, h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float uv[2];
            if (fread(uv, 4, 2, f) != 2) { fprintf(stderr, "short flo\n"); exit(2); }
            (*wx)->data[y * (*wx)->stride + x] = uv[0];
            (*wy)->data[y * (*wy)->stride + x] = uv[1];
        }
    fclose(f);
}

static void write_flo(const char *path, const image_t *wx, const image_t *wy) {
    FILE *f = fopen(path, "wb");
    float tag = 202021.25f;
    fwrite(&tag, 4, 1, f); fwrite(&wx->width, 4, 1, f); fwrite(&wx->height, 4, 1, f);
    for (int y = 0; y < wx->height; y++)
        for (int x = 0; x < wx->width; x++) {
            float uv[2] = {wx->data[y * wx->stride + x], wy->data[y * wy->stride + x]};
            fwrite(uv, 4, 2, f);
        }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc != 13) { fprintf(stderr, "usage: a.ppm b.ppm in.flo out.flo alpha gamma delta sigma outer inner solver omega\n"); return 2; }
    color_image_t *im1 = read_ppm(argv[1]), *im2 = read_ppm(argv[2]);
    image_t *wx, *wy;
    read_flo(argv[3], &wx, &wy);
    variational_params_t p;
    p.alpha = atof(argv[5]); p.gamma = atof(argv[6]); p.delta = atof(argv[7]); p.sigma = atof(argv[8]);
    p.niter_outer = atoi(argv[9]); p.niter_inner = atoi(argv[10]); p.niter_solver = atoi(argv[11]);
    p.sor_omega = atof(argv[12]);
    variational(wx, wy, im1, im2, &p);
    write_flo(argv[4], wx, wy);
    return 0;
}
"""


def read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(maxsplit=4)
    assert parts[0] == b"P6" and int(parts[3]) == 255
    w, h = int(parts[1]), int(parts[2])
    return np.frombuffer(parts[4][: w * h * 3], np.uint8).reshape(h, w, 3)


def write_ppm(path, img):
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def read_flo(path):
    with open(path, "rb") as f:
        tag, = np.fromfile(f, np.float32, 1)
        assert tag == 202021.25
        w, h = np.fromfile(f, np.int32, 2)
        return np.fromfile(f, np.float32, int(w) * int(h) * 2).reshape(int(h), int(w), 2)


def write_flo(path, flow):
    flow = np.ascontiguousarray(flow, np.float32)
    with open(path, "wb") as f:
        np.array([202021.25], np.float32).tofile(f)
        np.array([flow.shape[1], flow.shape[0]], np.int32).tofile(f)
        flow.tofile(f)


def sample_grid(h, w, step=GRID_STEP):
    """Rows and columns where the outputs are stored: every `step`-th one and the last one."""
    return np.unique(np.r_[np.arange(0, h, step), h - 1]), np.unique(np.r_[np.arange(0, w, step), w - 1])


def init_from(gt, q):
    """A perturbed init: ground truth + q / 2 (q int8), one float32 rounding."""
    return gt.astype(np.float32) + q.astype(np.float32) * np.float32(0.5)


def network_like(gt):
    """Ground truth box-downsampled x4 (edge-replicated to a multiple of 4) and bilinearly upsampled back."""
    h, w = gt.shape[:2]
    hp, wp = -(-h // 4) * 4, -(-w // 4) * 4
    g = np.pad(gt.astype(np.float64), ((0, hp - h), (0, wp - w), (0, 0)), mode="edge")
    small = g.reshape(hp // 4, 4, wp // 4, 4, 2).mean((1, 3))
    ys = np.clip((np.arange(h) + 0.5) / 4 - 0.5, 0, small.shape[0] - 1)
    xs = np.clip((np.arange(w) + 0.5) / 4 - 0.5, 0, small.shape[1] - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, small.shape[0] - 1), np.minimum(x0 + 1, small.shape[1] - 1)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = small[y0][:, x0] * (1 - fx) + small[y0][:, x1] * fx
    bot = small[y1][:, x0] * (1 - fx) + small[y1][:, x1] * fx
    return (top * (1 - fy) + bot * fy).astype(np.float32)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference sources at %s" % REF)
    rng = np.random.default_rng(20261016)
    a = read_ppm(os.path.join(SAMPLES, "0img0.ppm"))
    b = read_ppm(os.path.join(SAMPLES, "0img1.ppm"))
    gt = read_flo(os.path.join(SAMPLES, "0flow.flo"))
    y0, x0, ch, cw = CROP
    ca, cb, cgt = a[y0:y0 + ch, x0:x0 + cw], b[y0:y0 + ch, x0:x0 + cw], gt[y0:y0 + ch, x0:x0 + cw]

    def perturbation(shape):  # N(0, 0.75 px) in half pixels
        return np.clip(np.round(rng.normal(0.0, 0.75, shape) * 2), -127, 127).astype(np.int8)

    full_q, crop_q = perturbation(gt.shape), perturbation(cgt.shape)
    crop_init = init_from(cgt, crop_q)
    cases = [
        ("full", a, b, init_from(gt, full_q), DEFAULTS),
        ("crop", ca, cb, crop_init, DEFAULTS),
        ("crop_net", ca, cb, network_like(cgt).astype(np.float16).astype(np.float32), DEFAULTS),
        ("crop_o1s1", ca, cb, crop_init, dict(DEFAULTS, niter_outer=1, niter_solver=1)),
        ("crop_o1s30", ca, cb, crop_init, dict(DEFAULTS, niter_outer=1, niter_solver=30)),
        ("crop_kitti", ca, cb, crop_init, KITTI),
    ]
    out = {"cases": np.array([c[0] for c in cases]), "crop": np.array(CROP), "grid_step": np.array(GRID_STEP),
           "full_q": full_q, "crop_q": crop_q}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "driver.c")
        with open(src, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "variational_driver")
        subprocess.run(["gcc", "-O3", "-msse4", "-I", REF, src] +
                       [os.path.join(REF, s) for s in ("variational.c", "variational_aux.c", "solver.c", "image.c")] +
                       ["-lm", "-o", exe], check=True)
        for name, ia, ib, init, p in cases:
            pa, pb = os.path.join(tmp, name + "_a.ppm"), os.path.join(tmp, name + "_b.ppm")
            fi, fo = os.path.join(tmp, name + "_in.flo"), os.path.join(tmp, name + "_out.flo")
            write_ppm(pa, ia)
            write_ppm(pb, ib)
            write_flo(fi, init)
            args = [repr(float(np.float32(p[k]))) for k in ("alpha", "gamma", "delta", "sigma")]
            args += [str(p[k]) for k in ("niter_outer", "niter_inner", "niter_solver")]
            args += [repr(float(np.float32(p["sor_omega"])))]
            subprocess.run([exe, pa, pb, fi, fo] + args, check=True)
            res = read_flo(fo)
            print("%-11s %dx%d  mean |out - init| = %.4f px" % (name, ia.shape[1], ia.shape[0],
                                                                 float(np.abs(res - init).mean())))
            if name == "crop_net":
                out[name + "_init"] = init.astype(np.float16)  # exact: the init holds fp16 values
            rows, cols = sample_grid(*res.shape[:2])
            out[name + "_out"] = res[rows][:, cols]
            out[name + "_params"] = np.array([p[k] for k in ("alpha", "gamma", "delta", "sigma", "niter_outer",
                                                             "niter_inner", "niter_solver", "sor_omega")], np.float64)
    dst = os.path.join(HERE, "variational_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%.2f MB)" % (dst, os.path.getsize(dst) / 1e6))


if __name__ == "__main__":
    main()
