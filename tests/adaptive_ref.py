"""Adaptive sampling restated in numpy from the definition at the top of csrc/spt_adaptive.h: the selection of a
round, the mean and the resolve of an uneven accumulation, and a host emulation of a whole run. Test
infrastructure: tests/test_adaptive_host.py ties csrc/spt_adaptive.h's functions to it."""
import numpy as np

F = np.float32

# The run the host tests emulate: WARMUP uniform batches of BATCH frames, then ROUNDS adaptive rounds
# of BATCH frames, the header's default window (radius 1) and min_batches.
BATCH, WARMUP, ROUNDS = 4, 4, 12
# rel_error per scene, found on the CPU (tests/test_adaptive_host.py test_invariant_on_the_oracle asserts what they
# were chosen for): the emulated run ends with between 20 % and 80 % of the live pixels retired, at three or more
# distinct frame counts. C1 64 x 64 at 4 bounces and Cornell 96 x 54 (and 97 x 53) at 8.
REL_ERROR = {"c1": 0.025, "cornell": 0.4}


def select(e2, stop, batches, frames, rel_error, radius=1, min_batches=4):
    """One selection over (h, w) images: the bool image of the active pixels that keep tracing."""
    e2, stop = np.asarray(e2, dtype=F), np.asarray(stop, dtype=np.uint32)
    h, w = e2.shape
    active = stop == 0
    if batches < min_batches:
        return active.copy()
    t2 = F(rel_error) * F(rel_error)
    with np.errstate(invalid="ignore"):
        votes = active & ~(e2 <= t2)
    padded = np.zeros((h + 2 * radius, w + 2 * radius), dtype=bool)
    padded[radius:radius + h, radius:radius + w] = votes
    any_vote = np.zeros((h, w), dtype=bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            any_vote |= padded[dy:dy + h, dx:dx + w]
    return active & any_vote


def mean(accum):
    """(r / w, g / w, b / w, w) per pixel; zeros where w == 0."""
    a = np.asarray(accum, dtype=F)
    out = np.zeros_like(a)
    w = a[..., 3]
    some = w != 0
    with np.errstate(all="ignore"):
        for k in range(3):
            out[..., k] = np.where(some, a[..., k] / w, F(0))
    out[..., 3] = np.where(some, w, F(0))
    return out


def _u8(c):
    with np.errstate(invalid="ignore"):
        c = np.where(c < 0, F(0), np.where(c > 1, F(1), c)).astype(F)
    c = np.where(np.isnan(c), F(0), c).astype(F)
    return (c * F(255.0)).astype(np.uint8).astype(np.uint32)


def resolve(accum, exposure=1.0):
    """The RGBA8 word per pixel: k_resolve's expression with the pixel's own accum.w as the frame count."""
    a = np.asarray(accum, dtype=F).reshape(-1, 4)
    w = a[:, 3]
    with np.errstate(all="ignore"):
        ch = [_u8((a[:, k] / w).astype(F) * F(exposure)) for k in range(3)]
        alpha = _u8((w / w).astype(F))
    return (ch[0] << 24) | (ch[1] << 16) | (ch[2] << 8) | alpha


class Run:
    """The host emulation of an adaptive run: the state after the warm-up batches, then one round() per adaptive
    round. The fold is the library's (spt: the package; spt_noise_update_host, spt_noise_meter_host), the selection
    is `selector(e2, stop, batches, frames, rel_error, radius, min_batches)` -> bool image (default: select above).
    `constant`: the bool image of the pixels the run never traces."""

    def __init__(self, spt, moments, batches, frames, constant, rel_error, radius=1, min_batches=4, dark_floor=0.01,
                 selector=None):
        self.spt = spt
        self.moments = np.array(moments, dtype=F)
        self.batches, self.frames = int(batches), int(frames)
        self.rel_error, self.radius, self.min_batches, self.dark_floor = rel_error, radius, min_batches, dark_floor
        self.selector = selector if selector is not None else select
        self.stop = np.where(constant, np.uint32(frames), np.uint32(0)).astype(np.uint32)
        self.e2 = np.zeros(self.stop.shape, dtype=F)

    @property
    def active(self):
        return self.stop == 0

    def round(self, accum_after, n_frames):
        """Fold and select with the accumulation after the round's frames (only its active pixels are read).
        Returns the number of pixels still active."""
        spt, active = self.spt, self.active
        folded = spt.noise_update_host(accum_after, float(n_frames), float(self.frames), self.moments)
        self.moments[active] = folded[active]
        self.batches += 1
        self.frames += n_frames
        p = spt.NoiseParams(radius=0, dark_floor=self.dark_floor)
        _, e2 = spt.noise_meter_host(self.moments, self.batches, float(self.frames), p)
        self.e2[active] = e2[active]
        keep = self.selector(self.e2, self.stop, self.batches, self.frames, self.rel_error, self.radius, self.min_batches)
        self.stop[active & ~keep] = self.frames
        return int(keep.sum())

    def counts(self):
        """The frames each pixel holds: stop for a retired one, the run's frame count for an active one."""
        return np.where(self.active, np.uint32(self.frames), self.stop)
