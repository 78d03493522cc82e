"""EpicFlow variational refinement on the GPU (src.variational.refine) on the paths variational_golden.npz never
reaches, against the reference binary's outputs in tests/golden/variational_edges_golden.npz: the colour data term,
systems built around a non-zero increment, every smoothing order class, the narrowest and shortest images, the
readable solver, the SOR launch shapes of tall images, flows that leave the frame, and non-default alpha / omega.

Inputs are rebuilt from the committed samples by the generator's own case_inputs().  Every pixel is compared.  The
bounds are the project's accepted EPE tolerances, scaled up only as far as the REFERENCE's answer for the case moves
more under a one-ulp nudge of its init than its answer for the `crop` case does (`<name>_spread` / `crop_spread`,
both measured by the generator on the reference alone); the maximum is bounded as the p99.9 is.  With the committed
fixture every such ratio is below 1 (two of `crop`'s init pixels sit on the in-image mask's edge and dominate its
spread), so the bounds are in effect constants: mean < 1e-4 px, p99.9 < 2e-3 px, max < 2e-3 px for every case.

`far_edge` is not a regime of its own: it is `far` with ten inits exactly ON the frame's border, the one place where
the mask's `<=` and a `<` differ, which the other cases avoid because the reference's answer jumps there under a
nudge."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_variational_edges as gen  # noqa: E402

MEAN_TOL, P999_TOL = 1e-4, 2e-3  # test_gpu_variational.py
CASES = gen.CASE_NAMES           # pinned against the issue's table by test_variational_cpu.py


class Edges:
    def __init__(self, golden_dir):
        self.gen = gen
        self.samples = gen.load_samples(os.path.join(golden_dir, "samples"))
        with np.load(os.path.join(golden_dir, gen.FIXTURE)) as z:
            self.z = {k: z[k] for k in z.files}
        for v in self.z.values():
            v.setflags(write=False)

    def inputs(self, name):
        return self.gen.case_inputs(name, self.samples, self.z)

    def bounds(self, name):
        """(mean, p99.9, max) bounds of a case, from the reference's one-ulp spreads alone."""
        s, c = self.z[name + "_spread"], self.z["crop_spread"]
        return (MEAN_TOL * max(1.0, s[0] / c[0]), P999_TOL * max(1.0, s[1] / c[1]), P999_TOL * max(1.0, s[2] / c[1]))

    def check(self, label, name, got):
        want = self.z[name + "_out"]
        assert got.shape == want.shape and np.isfinite(got).all()
        stats, bounds = self.gen.epe_stats(got, want), self.bounds(name)
        print("%s: EPE vs reference mean %.2e  p99.9 %.2e  max %.2e px  (bounds %.2e  %.2e  %.2e)"
              % ((label,) + stats + bounds))
        assert stats[0] < bounds[0] and stats[1] < bounds[1] and stats[2] < bounds[2], (stats, bounds)


@pytest.fixture(scope="module")
def edges(golden_dir):
    return Edges(golden_dir)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_case_list_is_the_fixture(edges):
    assert CASES == list(edges.z["cases"])


@pytest.mark.parametrize("name", CASES)
def test_matches_reference_binary(edges, name):
    from src.variational import refine
    a, b, init, p = edges.inputs(name)
    got = refine(dev(init), dev(a), dev(b), **p).cpu().numpy()
    edges.check(name, name, got)


def test_row_is_the_transposed_column(edges):
    """H = 1, where the reference reads out of bounds: the 1x40 transpose of `col` with the init's components
    swapped is the same one-pixel line swept in the same order, so its result, transposed and swapped back, is the
    `col` golden up to summation order."""
    from src.variational import refine
    a, b, init, p = edges.inputs("col")
    assert init.shape == (40, 1, 2)
    ta, tb, ti = a.transpose(1, 0, 2), b.transpose(1, 0, 2), init.transpose(1, 0, 2)[..., ::-1]
    got = refine(dev(ti), dev(ta), dev(tb), **p).cpu().numpy()
    assert got.shape == (1, 40, 2)
    edges.check("row", "col", got.transpose(1, 0, 2)[..., ::-1])


def test_tall_batch_equals_single_calls(edges):
    """Two 1100x12 pairs in one call (per-pair offsets into the skewed system at a large plane size): each is the
    bits of its single call."""
    from src.variational import refine
    a, b, init, p = edges.inputs("tall")
    pairs = [(a, b, init), (b, a, -init)]
    singles = [refine(dev(f), dev(x), dev(y), **p).cpu().numpy() for x, y, f in pairs]
    batch = refine(dev(np.stack([q[2] for q in pairs])), dev(np.stack([q[0] for q in pairs])),
                   dev(np.stack([q[1] for q in pairs])), **p).cpu().numpy()
    for i, s in enumerate(singles):
        assert np.array_equal(batch[i], s), i
    assert not np.array_equal(singles[0], singles[1])
