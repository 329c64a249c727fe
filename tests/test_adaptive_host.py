"""Adaptive sampling's per-pixel definition on the host (no GPU): csrc/spt_adaptive.h's functions, compiled as plain
C++ with AddressSanitizer and UndefinedBehaviorSanitizer into a program of its own (tests/cpp/adaptive_host_check.cpp),
against the numpy restatement (tests/adaptive_ref.py) on crafted images; then a whole run emulated on the CPU oracle's
frames with that program's selections, whose invariant — a pixel that stopped at n frames holds, bit for bit, the
oracle's accumulation of its first n frames — is what kernels built on the header will be tested by.

Figures of the emulated runs (4 warm-up batches and 12 rounds of 4 frames, radius 1; RMS error of the mean colour
over the live pixels against the oracle's 2048-frame mean; "uniform" is the oracle's render of as many frames as
the adaptive run's paths pay for on every live pixel):
  C1 64 x 64, 4 bounces, rel_error 0.025:     52.3 % of the live pixels retired, 80.4 % of the uniform run's paths;
                                              RMS adaptive 0.02147, uniform at equal paths (51 frames) 0.02323
  Cornell 96 x 54, 8 bounces, rel_error 0.4:  48.5 % retired, 78.6 % of the paths;
                                              RMS adaptive 0.1894, uniform at equal paths (50 frames) 0.2030
The adaptive image is the better of the two at equal paths on both scenes, by 7 to 8 %."""
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import host_program

F = np.float32
RADII = [0, 1, 2]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The header's functions under the sanitizers: run(e2, stop, batches, frames, rel_error, radius, min_batches,
    accum, exposure) -> (keep, mean, words), or None where the program refuses the parameters."""
    tmp = tmp_path_factory.mktemp("adaptive")
    exe = host_program.build("adaptive_host_check", tmp, with_host=False)  # (the header alone)

    def run(e2, stop, batches, frames, rel_error=0.1, radius=1, min_batches=4, accum=None, exposure=1.0):
        e2 = np.ascontiguousarray(e2, dtype=F)
        stop = np.ascontiguousarray(stop, dtype=np.uint32)
        h, w = e2.shape
        n = w * h
        accum = np.ones((n, 4), dtype=F) if accum is None else np.ascontiguousarray(accum, dtype=F).reshape(n, 4)
        inp, out = tmp / "in.bin", tmp / "out.bin"
        with open(inp, "wb") as f:
            np.array([w, h, batches, frames, radius, min_batches], dtype=np.uint32).tofile(f)
            np.array([rel_error, exposure], dtype=F).tofile(f)
            e2.tofile(f)
            stop.tofile(f)
            accum.tofile(f)
        r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=300)
        if r.returncode == 3:
            return None
        assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
        raw = np.fromfile(out, dtype=np.uint8)
        assert raw.size == 21 * n
        return (raw[:n].astype(bool).reshape(h, w), raw[n:17 * n].view(F).reshape(n, 4), raw[17 * n:].view(np.uint32))

    return run


def both(program, e2, stop, batches, frames, rel_error=0.1, radius=1, min_batches=4):
    """The header's selection, checked against the restatement."""
    got = program(e2, stop, batches, frames, rel_error, radius, min_batches)[0]
    want = ar.select(e2, stop, batches, frames, rel_error, radius, min_batches)
    assert np.array_equal(got, want), (radius, np.argwhere(got != want)[:4])
    return got


def crafted(w, h, seed, rel_error=0.1):
    """e2 around the target with every special value somewhere, and a third of the pixels retired."""
    rng = np.random.default_rng(seed)
    t2 = F(rel_error) * F(rel_error)
    e2 = (t2 * np.exp2(rng.uniform(-2, 2, (h, w)))).astype(F)
    special = np.array([NAN, INF, -INF, 0.0, -0.0, t2, np.nextafter(t2, F(0)), np.nextafter(t2, F(1))], dtype=F)
    flat = e2.reshape(-1)
    at = rng.integers(0, flat.size, special.size)
    flat[at] = special[:at.size]
    stop = np.where(rng.random((h, w)) < 0.33, np.uint32(12), np.uint32(0)).astype(np.uint32)
    return e2, stop


# ---- the selection on crafted images ------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (65, 3)])
def test_select_sizes(program, w, h, radius):
    """1 x 1: one tap; a row and a column: windows clipped on two sides; 65 x 3: every window clipped."""
    for seed in range(2):
        e2, stop = crafted(w, h, seed * 100 + w * 10 + h)
        keep = both(program, e2, stop, 5, 20, radius=radius)
        assert not np.any(keep & (stop != 0))  # a retired pixel never comes back
    # all active and all above the target: everything keeps; all at the target: nothing does
    stop = np.zeros((h, w), dtype=np.uint32)
    assert both(program, np.full((h, w), 1.0, dtype=F), stop, 5, 20, radius=radius).all()
    assert not both(program, np.full((h, w), F(0.1) * F(0.1), dtype=F), stop, 5, 20, radius=radius).any()


def test_select_special_values(program):
    """Radius 0, a pixel's own value decides: NaN and +inf keep; -inf, 0, -0, the target itself and the float below
    it retire; the float above the target keeps."""
    rel = 0.1
    t2 = F(rel) * F(rel)
    e2 = np.array([[NAN, INF, -INF, 0.0, -0.0, t2, np.nextafter(t2, F(0)), np.nextafter(t2, F(1))]], dtype=F)
    keep = both(program, e2, np.zeros(e2.shape, dtype=np.uint32), 4, 16, rel_error=rel, radius=0)
    assert keep.tolist() == [[True, True, False, False, False, False, False, True]]
    # the target is rel_error * rel_error in fp32, not the double's square rounded
    rel = 0.3
    t2 = F(rel) * F(rel)
    e2 = np.array([[t2, np.nextafter(t2, F(1))]], dtype=F)
    assert both(program, e2, np.zeros((1, 2), dtype=np.uint32), 4, 16, rel_error=rel, radius=0).tolist() == [[False, True]]


@pytest.mark.parametrize("radius", [1, 2])
def test_select_neighbours_vote_only_while_active(program, radius):
    """A quiet active pixel beside a noisy one: the noisy neighbour keeps it tracing while it is active, and does
    not once it has retired; a NaN neighbour votes like a noisy one."""
    n = 2 * radius + 3
    for noisy in (1.0, NAN, INF):
        e2 = np.zeros((1, n), dtype=F)
        e2[0, n // 2] = noisy
        stop = np.zeros((1, n), dtype=np.uint32)
        keep = both(program, e2, stop, 5, 20, radius=radius)[0]
        want = [abs(x - n // 2) <= radius for x in range(n)]
        assert keep.tolist() == want, ("an active neighbour above the target must vote", noisy)
        stop[0, n // 2] = 16
        keep = both(program, e2, stop, 5, 20, radius=radius)[0]
        assert not keep.any(), ("a retired neighbour above the target must not vote", noisy)
    # rows are neighbours as columns are
    e2 = np.zeros((n, n), dtype=F)
    e2[n // 2, n // 2] = 1.0
    keep = both(program, e2, np.zeros((n, n), dtype=np.uint32), 5, 20, radius=radius)
    yy, xx = np.mgrid[0:n, 0:n]
    assert np.array_equal(keep, (abs(yy - n // 2) <= radius) & (abs(xx - n // 2) <= radius))


def test_select_before_min_batches_keeps_every_active_pixel(program):
    e2, stop = crafted(17, 9, 3)
    e2[:] = 0.0
    for batches, min_batches in ((3, 4), (1, 2), (7, 8)):
        keep = both(program, e2, stop, batches, 20, min_batches=min_batches)
        assert np.array_equal(keep, stop == 0)
    assert not both(program, e2, stop, 4, 20, min_batches=4).any()


def test_validation(program):
    e2 = np.zeros((3, 4), dtype=F)
    stop = np.zeros((3, 4), dtype=np.uint32)
    assert program(e2, stop, 4, 16) is not None
    for kw in (dict(rel_error=0.0), dict(rel_error=-0.1), dict(rel_error=NAN), dict(rel_error=INF), dict(radius=3),
               dict(min_batches=1), dict(min_batches=0)):
        assert program(e2, stop, 4, 16, **kw) is None, kw
    for batches, frames in ((0, 16), (4, 0), (4, 2 ** 24 + 1)):
        assert program(e2, stop, batches, frames) is None, (batches, frames)


# ---- mean and resolve ---------------------------------------------------------------------------------------
def uneven_accum(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 4), dtype=F)
    a[:, 3] = rng.integers(1, 65, n).astype(F)
    a[:, :3] = (rng.uniform(0.0, 1.6, (n, 3)) * a[:, 3:4]).astype(F)
    a[0] = (0.0, 0.0, 0.0, 0.0)        # no frames
    a[1] = (1.0, 2.0, 3.0, 0.0)        # ... with sums: still zeros
    a[2] = (NAN, INF, -1.0, 8.0)
    a[3] = (8.0, 4.0, 0.0, 8.0)
    return a


def test_mean_and_resolve(spt, program):
    a = uneven_accum(300, 1)
    zeros = np.zeros((1, 300), dtype=F)
    for exposure in (1.0, 0.37, 2.5):
        _, m, words = program(zeros, zeros.astype(np.uint32), 4, 16, accum=a, exposure=exposure)
        want = ar.mean(a)
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(m)) and np.array_equal(m[~nan].view(np.uint32), want[~nan].view(np.uint32))
        assert np.array_equal(words, ar.resolve(a, exposure)), exposure
    _, m, words = program(zeros, zeros.astype(np.uint32), 4, 16, accum=a)
    assert np.all(m[:2] == 0) and m[3].tolist() == [1.0, 0.5, 0.0, 8.0]
    assert words[0] == 0 and words[3] == 0xFF7F00FF and words[2] == 0x00FF00FF
    # an even accumulation: the resolve over one frame count (spt_display_host with the clamp operator is
    # spt_resolve_rgba8_exposure's expression)
    a[:, 3] = 16.0
    for exposure in (1.0, 0.8):
        d = spt.Display(exposure=exposure, tonemap=spt.TONEMAP_CLAMP)
        words = program(zeros, zeros.astype(np.uint32), 4, 16, accum=a, exposure=exposure)[2]
        assert np.array_equal(words, spt.display_host(a, d, 16.0))


# ---- a run emulated on the oracle ---------------------------------------------------------------------------
_cache = {}


def oracle_run(spt, ref, program, name, w, h, bounces, rel_error=None):
    """The run of adaptive_ref (WARMUP batches, ROUNDS rounds of BATCH frames) emulated on the oracle's per-frame
    images, every selection made by the program and checked against the restatement. Constant pixels: those whose
    warm-up frames are all the same bits."""
    key = (name, w, h, bounces, rel_error)
    if key in _cache:
        return _cache[key]
    rs = ref.RefScene(*spt.build_scene(name))
    total = ar.BATCH * (ar.WARMUP + ar.ROUNDS)
    frames = [rs.render(w, h, k, 1, bounces, 2, 0, threads=8) for k in range(total)]
    acc = np.zeros((h, w, 4), dtype=F)
    m, k = None, 0
    for _ in range(ar.WARMUP):
        for _ in range(ar.BATCH):
            acc = acc + frames[k]
            k += 1
        m = spt.noise_update_host(acc, ar.BATCH, k - ar.BATCH, m)
    first = frames[0].view(np.uint32)
    constant = np.all([np.all(f.view(np.uint32) == first, axis=-1) for f in frames[:k]], axis=0)
    run = ar.Run(spt, m, ar.WARMUP, k, constant, ar.REL_ERROR[name] if rel_error is None else rel_error,
                 selector=lambda *a: both(program, *a))
    paths = int((~constant).sum()) * k
    for _ in range(ar.ROUNDS):
        active = run.active
        paths += int(active.sum()) * ar.BATCH
        for _ in range(ar.BATCH):
            acc[active] = acc[active] + frames[k][active]
            k += 1
        run.round(acc, ar.BATCH)
    _cache[key] = (rs, run, acc, constant, paths)
    return _cache[key]


@pytest.mark.parametrize("name,w,h,bounces", [("c1", 64, 64, 4), ("cornell", 96, 54, 8)])
def test_invariant_on_the_oracle(spt, ref, program, name, w, h, bounces):
    rs, run, acc, constant, paths = oracle_run(spt, ref, program, name, w, h, bounces)
    live = ~constant
    total = ar.BATCH * (ar.WARMUP + ar.ROUNDS)
    counts = run.counts()
    assert np.array_equal(acc[..., 3], counts.astype(F))
    # every pixel holds the oracle's accumulation of its first counts[p] frames, bit for bit
    for fc in np.unique(counts):
        want = rs.render(w, h, 0, int(fc), bounces, 2, 0, threads=8)
        at = counts == fc
        assert np.array_equal(acc[at].view(np.uint32), want[at].view(np.uint32)), (name, int(fc))
    # what rel_error was chosen for
    retired = ~run.active & live
    share = retired.sum() / live.sum()
    distinct = np.unique(run.stop[retired])
    print(f"adaptive {name} {w}x{h}: {live.sum()} live, {retired.sum()} retired ({share:.3f}), at {distinct.tolist()}")
    assert 0.2 <= share <= 0.8 and distinct.size >= 3
    assert np.all(run.stop[constant] == ar.BATCH * ar.WARMUP)
    # fewer paths than the uniform run of equal length; every retired pixel's frozen e2 is at the target or below
    assert paths < int(live.sum()) * total
    t2 = F(ar.REL_ERROR[name]) * F(ar.REL_ERROR[name])
    assert np.all(run.e2[retired] <= t2)
    # quality, recorded (the module's docstring): not asserted
    truth = rs.render(w, h, 0, 2048, bounces, 2, 0, threads=8).astype(np.float64)[..., :3] / 2048.0
    equal = max(1, paths // int(live.sum()))
    uniform = rs.render(w, h, 0, equal, bounces, 2, 0, threads=8).astype(np.float64)[..., :3] / equal
    adaptive = acc.astype(np.float64)[..., :3] / acc[..., 3:4]

    def rms(img):
        return float(np.sqrt(np.mean(np.sum((img[live] - truth[live]) ** 2, axis=-1))))

    print(f"adaptive {name}: paths {paths} of {int(live.sum()) * total} ({paths / (live.sum() * total):.3f}); "
          f"RMS adaptive {rms(adaptive):.4g}, uniform at equal paths ({equal} frames) {rms(uniform):.4g}")


def test_tiny_and_huge_targets(spt, ref, program):
    """rel_error 1e-30: nothing retires but the constant pixels; 1e30: every live pixel retires in the first round."""
    _, run, acc, constant, _ = oracle_run(spt, ref, program, "c1", 64, 64, 4, rel_error=1.0e-30)
    total, warm = ar.BATCH * (ar.WARMUP + ar.ROUNDS), ar.BATCH * ar.WARMUP
    assert np.array_equal(run.active, ~constant) and np.all(acc[~constant][:, 3] == total)
    # (a finite e2 against an infinite target: rel_error must be finite, its square need not be)
    _, run, acc, constant, _ = oracle_run(spt, ref, program, "c1", 64, 64, 4, rel_error=1.0e30)
    assert not run.active.any() and np.all(run.stop[~constant] == warm + ar.BATCH) and np.all(run.stop[constant] == warm)
