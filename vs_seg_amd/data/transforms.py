"""The reference's MONAI transform chains (ref:params/VSparams.py:205-245), restated and moved to the GPU.

Deterministic head (cached once per case, like `CacheDataset(cache_rate=1.0)`, ref:params/VSparams.py:305-334):
    LoadNiftid → AddChanneld → Orientationd("RAS") → NormalizeIntensityd(image) → SpatialPadd(pad_crop_shape)
Random tail (per sample, per epoch):
    RandFlipd(prob=0.5, spatial_axis=0) → RandSpatialCropd(roi=pad_crop_shape, random_center=True, random_size=False)

Optional training augmentation (off by default; this project's own conventions — MONAI's RandAffined / RandScaleIntensityd /
RandShiftIntensityd / RandGaussianNoised are the transforms it corresponds to): an in-plane rotation and scaling about the centre
of the crop window, a gain, a bias and Gaussian noise, all applied by ONE `vsseg_crop_affine` launch in place of the crop.  Two more families
(MONAI's Rand3DElastic / RandBiasField, TorchIO's RandomElasticDeformation) are one smooth random B-spline field over the patch, a 2-vector for an
in-plane elastic deformation and a scalar for a multiplicative MR bias field; with either on, the launch is `vsseg_crop_field`, the same gather with the field.
Four appearance families act on the image after the crop launch, each per sample with probability `appearance_prob`: an in-plane Gaussian blur and a simulated
low-resolution acquisition (`vsseg_patch_filter`), then a contrast change and a gamma curve (`vsseg_patch_tone`; batchgenerators' ContrastAugmentation with
preserve_range, MONAI's RandAdjustContrast).
Three acquisition families act on the image between the crop launch and the appearance families, each per sample with probability `acquisition_prob`: thick slices along
z, phase-encode ghosting along x or y and a k-space spike (`vsseg_patch_acquisition`; TorchIO's RandomAnisotropy, RandomGhosting, RandomSpike).

The numpy restatement of MONAI 0.4.0's arithmetic that checks the HIP path (`vsseg_normalize_intensity`, `vsseg_crop_flip`) is test
infrastructure and lives in `oracle/data_oracle.py` (parity unpinned — MONAI is not installed).  `PatchSampler`
is the product path: cached volumes live in HBM, one launch crops/flips image and label of a whole batch.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import nifti

MAX_SEED = np.iinfo(np.uint32).max + 1


# ---------------------------------------------------------------------------------------------------------------
# geometry shared with the checker (the numpy restatement of the MONAI arithmetic lives in oracle/data_oracle.py: test infrastructure)
# ---------------------------------------------------------------------------------------------------------------
def pad_widths(shape: Sequence[int], spatial_size: Sequence[int]) -> List[Tuple[int, int]]:
    """SpatialPadd(method="symmetric"): width w = max(target - size, 0) split as (w // 2, w - w // 2)."""
    out = []
    for d, t in zip(shape, spatial_size):
        w = max(int(t) - int(d), 0)
        out.append((w // 2, w - w // 2))
    return out


def _bind(defaults: Dict, values: Sequence, named: Dict, what: str) -> Dict:
    """`values`, then `named`, over `defaults`, as a Python call binds them: TypeError for too many values, an unknown name and a name given twice."""
    if len(values) > len(defaults):
        raise TypeError(f"{what} takes at most {len(defaults)} positional ranges ({len(values)} given)")
    given = dict(zip(defaults, values))
    for k in named:
        if k not in defaults or k in given:
            raise TypeError(f"{what} got " + ("multiple values for argument" if k in given else "an unexpected keyword argument") + f" '{k}'")
    return {**defaults, **given, **named}


def _augment_rules(a, raw):
    if a["rotate_deg"] > 180.0:
        raise ValueError(f"rotate_deg = {a['rotate_deg']}: at most 180")
    for k in ("scale", "intensity_scale"):
        if a[k] >= 1.0:
            raise ValueError(f"{k} = {a[k]}: must be < 1 (the factor 1 + u stays positive)")


def _field_rules(a, raw):
    """The in-plane control-point spacing is an integer >= 1 (returned as an int); elastic_mag <= field_spacing / 4 (beyond it the deformation could fold: vsseg_hip.h)."""
    sp = float(raw["field_spacing"])
    if not (np.isfinite(sp) and sp >= 1.0 and sp == int(sp)):
        raise ValueError(f"field_spacing = {raw['field_spacing']}: must be an integer >= 1 (voxels)")
    if a["elastic_mag"] > sp / 4.0:
        raise ValueError(f"elastic_mag = {a['elastic_mag']}: at most field_spacing / 4 = {sp / 4.0} (the deformation must not fold)")
    a["field_spacing"] = int(sp)


def _appearance_rules(a, raw):
    if a["blur_sigma"] > 1.5:
        raise ValueError(f"blur_sigma = {a['blur_sigma']}: at most 1.5 in-plane voxels (a radius of 5)")
    if a["lowres"] != 0.0 and not 0.25 <= a["lowres"] < 1.0:
        raise ValueError(f"lowres = {a['lowres']}: 0 (off) or a resolution factor in [0.25, 1)")
    for k in ("contrast", "gamma"):
        if a[k] >= 1.0:
            raise ValueError(f"{k} = {a[k]}: must be < 1 (the factor 1 + u stays positive)")
    if a["appearance_prob"] > 1.0:
        raise ValueError(f"appearance_prob = {a['appearance_prob']}: a probability, at most 1")


def _acquisition_rules(a, raw):
    """thick_slices 0 or an integer in 2..4 (the largest slab height in voxels along z: 4 x 1.5 mm = 6 mm slices; returned as an int), ghost <= 1 (the largest
    attenuation of the ghosted k-space lines), acquisition_prob <= 1; spike is the largest amplitude in standard deviations of the normalised image."""
    if a["thick_slices"] != int(a["thick_slices"]) or int(a["thick_slices"]) not in (0, 2, 3, 4):
        raise ValueError(f"thick_slices = {raw['thick_slices']}: 0 (off) or an integer slab height in 2..4 voxels")
    a["thick_slices"] = int(a["thick_slices"])
    if a["ghost"] > 1.0:
        raise ValueError(f"ghost = {a['ghost']}: an attenuation, at most 1")
    if a["acquisition_prob"] > 1.0:
        raise ValueError(f"acquisition_prob = {a['acquisition_prob']}: a probability, at most 1")


@dataclass(frozen=True)
class Family:
    """One row of FAMILIES: everything between a flag and a launch that knows an augmentation family by name reads it from here."""

    name: str  # the attribute of RandomTail and the key of Augmentation.values that hold its validated arguments
    defaults: Dict[str, float]  # its arguments in positional order with their defaults (0 = off)
    ranges: Tuple[str, ...]  # those whose non-zero value switches the family on (a probability and field_spacing are no ranges)
    flag: str  # the attribute of RandomTail that says whether it is on
    rng: str  # the attribute of RandomTail that holds its RandomState (None while it is off)
    key: str  # the key it travels under in a transform description (VSparams.get_transforms, CachedLoader)
    rules: Callable[[Dict, Dict], None]  # its own rules beyond "finite and >= 0", over (the floats, the arguments as given)
    own: Tuple[str, ...] = ()  # arguments that only `rules` looks at and adds

    def check(self, *values, **named) -> Dict[str, float]:
        """The arguments as floats (or what `rules` makes of them), in positional order; ValueError for a negative or non-finite value and for what `rules` rejects."""
        raw = _bind(self.defaults, values, named, "check_" + self.key)
        a = {k: float(v) for k, v in raw.items() if k not in self.own}
        for k, v in a.items():
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"augmentation range {k} = {v}: must be finite and >= 0")
        self.rules(a, raw)
        return a


# In SEEDING ORDER: RandomTail seeds flip, crop, then one state per family that is on, in this order.  A family that is off draws no seed, so switching a family on never
# moves the draws of the families before it, and a new family goes LAST: that alone keeps the flips, crops and draws of every earlier training run reproducible.
FAMILIES = (
    Family("augment", dict(rotate_deg=0.0, scale=0.0, intensity_scale=0.0, intensity_shift=0.0, noise_std=0.0), ("rotate_deg", "scale", "intensity_scale", "intensity_shift", "noise_std"),
           "augmenting", "_augR", "augment", _augment_rules),
    Family("field", dict(elastic_mag=0.0, bias_field=0.0, field_spacing=64), ("elastic_mag", "bias_field"), "fielding", "_fieldR", "field_augment", _field_rules, own=("field_spacing",)),
    Family("appearance", dict(blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, appearance_prob=0.25), ("blur_sigma", "lowres", "contrast", "gamma"),
           "appearing", "_appR", "appearance_augment", _appearance_rules),
    Family("acquisition", dict(thick_slices=0, ghost=0.0, spike=0.0, acquisition_prob=0.25), ("thick_slices", "ghost", "spike"), "acquiring", "_acqR", "acquisition_augment", _acquisition_rules),
)
AUGMENT_KEYS, FIELD_KEYS, APPEARANCE_KEYS, ACQUISITION_KEYS = (tuple(f.defaults) for f in FAMILIES)
check_augment, check_field_augment, check_appearance_augment, check_acquisition_augment = (f.check for f in FAMILIES)
DEFAULTS = {k: v for f in FAMILIES for k, v in f.defaults.items()}  # every argument of every family, in table order
GHOST_COUNTS = (2, 3, 4, 6, 8)  # the ghost counts a sample may draw: those that divide the axis


@dataclass(frozen=True)
class Augmentation:
    """The validated arguments of every family, made once where they enter (a constructor, the command line) and handed on whole."""

    values: Dict[str, Dict[str, float]]  # Family.name -> what its `check` returned

    @classmethod
    def of(cls, *ranges, **named) -> "Augmentation":
        """From the arguments of all families in table order, by position, by name or both (a record is returned as it is); TypeError as a call, ValueError of a family."""
        if len(ranges) == 1 and isinstance(ranges[0], cls) and not named:
            return ranges[0]
        flat = _bind(DEFAULTS, ranges, named, "Augmentation.of")
        return cls({f.name: f.check(*(flat[k] for k in f.defaults)) for f in FAMILIES})

    def on(self, family: Family) -> bool:
        return any(self.values[family.name][k] != 0 for k in family.ranges)

    def flat(self) -> Dict[str, float]:
        return {k: v for d in self.values.values() for k, v in d.items()}




NEUTRAL_ACQUISITION = dict(thick=1, thick_offset=0, ghost_axis=0, ghosts=0, ghost_alpha=np.float32(0.0), spike_amp=np.float32(0.0), spike_k=(0, 0), spike_phase=np.float32(0.0))


def blur_taps(sigma: float) -> np.ndarray:
    """The R + 1 half-taps of `vsseg_filter_job.taps` for R = ceil(3 sigma): w_k = exp(-k^2 / (2 sigma^2)), normalised in fp64 so that w_0 + 2 sum_{k>=1} w_k = 1,
    rounded once to fp32.  sigma = 0: no taps (radius 0)."""
    sigma = float(sigma)
    if sigma == 0.0:
        return np.zeros(0, np.float32)
    w = np.exp(-np.arange(int(np.ceil(3.0 * sigma)) + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def coarse_size(roi: Sequence[int], f: float) -> Tuple[int, int]:
    """The in-plane sample counts of `vsseg_filter_job.coarse` at the resolution factor f: n_a = max(1, floor(roi_a * f + 0.5)); (roi_x, roi_y) means off."""
    return tuple(max(1, int(np.floor(int(roi[a]) * float(f) + 0.5))) for a in range(2))


def field_launch_spacing(field_spacing: int) -> Tuple[int, int, int]:
    """(S, S, max(1, (S + 2) // 4)): the lattice is roughly isotropic in millimetres over 0.4 x 0.4 x 1.5 mm voxels."""
    s = int(field_spacing)
    return s, s, max(1, (s + 2) // 4)


def affine_matrix(roi: Sequence[int], start: Sequence[int], sdim_x: int, flip: bool, angle: float = 0.0, scale: float = 1.0) -> np.ndarray:
    """fp32 3x4 matrix of `vsseg_affine_job.m`: output index p -> source voxel coordinate
        s = c_src + R_z(angle) diag(1/scale, 1/scale, 1) (p - c_roi),   c_roi = (roi - 1) / 2,   c_src = start + c_roi
    (the centre of the window the plain crop would take; rotation and scaling in-plane only: the voxels are 0.4 x 0.4 x 1.5 mm), then the x mirror
    s_x -> sdim_x - 1 - s_x on row 0.  Composed in fp64, rounded once.  angle = 0, scale = 1 gives [I | start] (or its mirrored form) exactly."""
    c_roi = (np.asarray(roi, np.float64) - 1.0) / 2.0
    c_src = np.asarray(start, np.float64) + c_roi
    c, s = np.cos(float(angle)), np.sin(float(angle))
    A = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag([1.0 / scale, 1.0 / scale, 1.0])
    m = np.concatenate([A, (c_src - A @ c_roi)[:, None]], 1)
    if flip:
        m[0] = -m[0]
        m[0, 3] += sdim_x - 1.0
    return (m + 0.0).astype(np.float32)  # + 0.0: no negative zeros


class RandomTail:
    """The random decisions of RandFlipd + RandSpatialCropd with MONAI's per-transform RandomState layout:
    `Compose.set_random_state(seed)` seeds its own state and gives every Randomizable transform, in order, the seed
    `R.randint(MAX_SEED, dtype=uint32)`; RandFlipd draws `R.random_sample() < prob`, RandSpatialCropd draws
    `R.randint(0, size - roi + 1)` per axis where size > roi.

    After those two, every family of FAMILIES that is on (a range non-zero) gets a state of its own, seeded from `R` in table order; one that is off draws no seed.  So
    flip, crop and every family earlier in the table draw the same with a family on or off.  `*ranges, **named` are the arguments of all families (Augmentation.of) or
    one Augmentation; per family the tail holds the validated dict (`augment`, `field`, `appearance`, `acquisition`), its on-flag (`augmenting`, ...) and its state.

    augment: `draw_augment()` draws per sample, in this order and only for the ranges that are non-zero: angle ~ U(-rotate_deg, rotate_deg), scale factor
    1 + U(-scale, scale), gain 1 + U(-intensity_scale, intensity_scale), bias ~ U(-intensity_shift, intensity_shift); `draw_noise_seed()` draws one randint(2^32) per
    batch when noise_std != 0.

    field: `draw_field_seed()` draws one randint(2^32) per batch (the high half of the launch seed: the lattice differs from batch to batch, noise or no noise);
    `draw_field()` draws per sample, in this order and only for the ranges that are non-zero: a ~ U(0, elastic_mag), beta ~ U(0, bias_field).

    appearance: `draw_appearance()` draws per sample, for each range that is non-zero, in the order blur, low resolution, contrast, gamma: first
    `random_sample() < appearance_prob`, then the value (sigma ~ U(S/2, S), f ~ U(F, 1), c ~ U(1 - C, 1 + C), gamma ~ U(1 - G, 1 + G)).  Both numbers are always
    drawn, so the position in the stream does not depend on the outcome; a range that is not hit gets its neutral value (sigma = 0, f = 1, c = 1, gamma = 1).

    acquisition: `draw_acquisition(roi)` draws per sample, for each range that is non-zero, in the order thick slices, ghosting, spike, and always all its numbers:
      thick   random_sample() < acquisition_prob, f = randint(2, F + 1), o = randint(0, 12) % f
      ghost   random_sample() < acquisition_prob, alpha = uniform(0, A), axis = randint(0, 2), r = randint(0, 120); n = cands[r % len(cands)] with cands the members of
              GHOST_COUNTS that divide roi[axis]; no candidate, or alpha == 0 in fp32: neutral
      spike   random_sample() < acquisition_prob, amp = uniform(0, S), kx = randint(0, rx), ky = randint(0, ry), phase = uniform(0, 2 pi); (kx, ky) == (0, 0), or
              amp == 0 in fp32: neutral
    The result has the fields of `vsseg_acquisition_job`; NEUTRAL_ACQUISITION is the job that copies."""

    def __init__(self, roi: Sequence[int], flip_prob: Optional[float] = 0.5, seed: Optional[int] = None, *ranges, **named):
        self.roi, self.flip_prob = tuple(int(r) for r in roi), flip_prob
        self.augmentation = Augmentation.of(*ranges, **named)
        for fam in FAMILIES:
            setattr(self, fam.name, self.augmentation.values[fam.name])
            setattr(self, fam.flag, self.augmentation.on(fam))
        self.set_random_state(seed)

    def set_random_state(self, seed: Optional[int] = None):
        R = np.random.RandomState(seed)
        state = lambda on: np.random.RandomState(R.randint(MAX_SEED, dtype="uint32")) if on else None  # noqa: E731
        self._flipR, self._cropR = state(self.flip_prob is not None), state(True)
        for fam in FAMILIES:
            setattr(self, fam.rng, state(getattr(self, fam.flag)))
        return self

    def draw(self, shape: Sequence[int]) -> Tuple[bool, Tuple[int, int, int]]:
        flip = bool(self._flipR.random_sample() < self.flip_prob) if self._flipR is not None else False
        start = tuple(int(self._cropR.randint(0, s - r + 1)) if s > r else 0 for s, r in zip(shape, self.roi))
        return flip, start

    def draw_augment(self) -> Tuple[float, float, float, float]:
        """(angle in radians, scale factor, gain, bias) of one sample."""
        a, u = self.augment, (lambda r: float(self._augR.uniform(-r, r)) if r != 0.0 else 0.0)
        return float(np.deg2rad(u(a["rotate_deg"]))), 1.0 + u(a["scale"]), 1.0 + u(a["intensity_scale"]), u(a["intensity_shift"])

    def draw_noise_seed(self) -> int:
        return int(self._augR.randint(MAX_SEED, dtype="uint32")) if self.augment["noise_std"] != 0.0 else 0

    def draw_field_seed(self) -> int:
        return int(self._fieldR.randint(MAX_SEED, dtype="uint32")) if self.fielding else 0

    def draw_field(self) -> Tuple[float, float]:
        """(elastic_mag in voxels, bias_log) of one sample."""
        f, u = self.field, (lambda r: float(self._fieldR.uniform(0.0, r)) if r != 0.0 else 0.0)
        return u(f["elastic_mag"]), u(f["bias_field"])

    def draw_appearance(self) -> Tuple[float, float, float, float]:
        """(blur sigma in in-plane voxels, resolution factor, contrast factor, gamma) of one sample; (0, 1, 1, 1) is neutral."""
        a, p = self.appearance, self.appearance["appearance_prob"]

        def family(rng, lo, hi, neutral):
            if rng == 0.0:
                return neutral
            hit, v = self._appR.random_sample() < p, float(self._appR.uniform(lo, hi))
            return v if hit else neutral

        return (family(a["blur_sigma"], a["blur_sigma"] / 2.0, a["blur_sigma"], 0.0), family(a["lowres"], a["lowres"], 1.0, 1.0),
                family(a["contrast"], 1.0 - a["contrast"], 1.0 + a["contrast"], 1.0), family(a["gamma"], 1.0 - a["gamma"], 1.0 + a["gamma"], 1.0))

    def draw_acquisition(self, roi: Optional[Sequence[int]] = None) -> Dict:
        """The fields of `vsseg_acquisition_job` for one sample of patch shape `roi` (default: the sampler's own)."""
        roi = self.roi if roi is None else tuple(int(r) for r in roi)
        a, p, R = self.acquisition, self.acquisition["acquisition_prob"], self._acqR
        job = dict(NEUTRAL_ACQUISITION)
        if a["thick_slices"]:
            hit, f, o = R.random_sample() < p, int(R.randint(2, a["thick_slices"] + 1)), int(R.randint(0, 12))
            if hit:
                job.update(thick=f, thick_offset=o % f)
        if a["ghost"] != 0.0:
            hit, alpha, axis, r = R.random_sample() < p, np.float32(R.uniform(0.0, a["ghost"])), int(R.randint(0, 2)), int(R.randint(0, 120))
            cands = [n for n in GHOST_COUNTS if roi[axis] % n == 0]
            if hit and cands and alpha != 0.0:
                job.update(ghost_axis=axis, ghosts=cands[r % len(cands)], ghost_alpha=alpha)
        if a["spike"] != 0.0:
            hit, amp, kx, ky, phase = R.random_sample() < p, np.float32(R.uniform(0.0, a["spike"])), int(R.randint(0, roi[0])), int(R.randint(0, roi[1])), np.float32(R.uniform(0.0, 2.0 * np.pi))
            if hit and (kx, ky) != (0, 0) and amp != 0.0:
                job.update(spike_amp=amp, spike_k=(kx, ky), spike_phase=phase)
        return job


# ---------------------------------------------------------------------------------------------------------------
# product path: cached volumes in HBM, HIP kernels
# ---------------------------------------------------------------------------------------------------------------
def load_case(files: Dict[str, str], pad_to: Optional[Sequence[int]] = None, device="cuda") -> Dict:
    """Deterministic head of the chain for one {"image": path, "label": path} entry → cached device tensors [X,Y,Z] fp32
    (RAS, image normalised on the GPU, both zero-padded to at least `pad_to`) + the metadata NIfTI export needs."""
    lib = L.lib()
    out: Dict = {"files": dict(files)}
    stream = torch.cuda.current_stream().cuda_stream
    for key in ("image", "label"):
        arr, aff, hdr = nifti.read_nifti(files[key])
        ras, ras_aff, ornt = nifti.to_ras(arr, aff)
        t = torch.from_numpy(np.ascontiguousarray(ras, dtype=np.float32)).to(device)
        if key == "image":
            acc = torch.zeros(2, dtype=torch.float64, device=device)
            y = torch.empty_like(t)
            L.check(lib.vsseg_normalize_intensity(t.data_ptr(), y.data_ptr(), t.numel(), acc.data_ptr(), stream), "normalize_intensity")
            t = y
        if pad_to is not None:
            pw = pad_widths(t.shape, pad_to)
            if any(a or b for a, b in pw):
                t = torch.nn.functional.pad(t, (pw[2][0], pw[2][1], pw[1][0], pw[1][1], pw[0][0], pw[0][1]))
        out[key] = t.contiguous()
        out[key + "_meta"] = dict(affine=ras_aff, original_affine=aff, ornt=ornt, filename_or_obj=files[key], spatial_shape=tuple(arr.shape))
    assert out["image"].shape == out["label"].shape, f"image/label shapes differ for {files}"
    return out


class PatchSampler:
    """RandFlipd + RandSpatialCropd over cached cases, one `vsseg_crop_flip` launch per batch.

    `sample(indices)` → (inputs [B,1,*roi], labels [B,1,*roi]) fp32 on the device, the tensors the reference's DataLoader
    yields as batch["image"], batch["label"] (ref:params/VSparams.py:455).  `flip_prob=None` = the validation chain
    (no RandFlipd, ref:params/VSparams.py:224-236).  `*ranges, **named` are RandomTail's; the tail gets the one validated record.  Draws within a batch: noise seed,
    field seed, then per sample flip / crop, augment, field; after the crop launch the acquisition draws per sample, then the appearance draws per sample.

    A non-zero `rotate_deg`, `scale`, `intensity_scale`, `intensity_shift` or `noise_std` (see RandomTail) replaces that launch by one
    `vsseg_crop_affine` launch: the image is resampled trilinearly and gets gain, bias and noise, the label goes through the same matrix
    with nearest-neighbour lookup.  `last_augment` then holds, per sample, what a test needs to replay the launch.

    A non-zero `elastic_mag` (voxels) or `bias_field` (log of the factor) makes that launch `vsseg_crop_field` with the lattice spacing
    `field_launch_spacing(field_spacing)`: image and label of a sample share the deformation, the bias field multiplies the image only.  `last_augment` then
    also holds `elastic_mag`, `bias_log` (fp32) and `spacing` per sample.  With both 0 the sampler takes the paths above, launch for launch.

    A non-zero `blur_sigma`, `lowres`, `contrast` or `gamma` with `appearance_prob` > 0 adds, after whichever crop launch it is and on the image only, one
    `vsseg_patch_filter` launch when a sample of the batch drew a blur or a low resolution and one `vsseg_patch_tone` launch when one drew a contrast or a gamma.
    `last_augment[b]` then also holds `blur_sigma` (as drawn), `blur_taps` (fp32, R + 1 values), `coarse` (two ints), `contrast` and `gamma` (fp32), and `last_tone_stats` the
    [B, 4] device tensor {min, max, mean, 0} of the tone launch (None when it was skipped).  The scratch of the filter and the workspace of the tone launch belong to
    the sampler; the filtered image is a new tensor, because it is handed to the caller.  Nothing here reads device memory from the host or synchronises.  With the
    four ranges 0, or `appearance_prob` 0, the sampler takes the paths above, launch for launch.

    A non-zero `thick_slices`, `ghost` or `spike` with `acquisition_prob` > 0 adds, after whichever crop launch it is, BEFORE the appearance launches and on the image
    only, one `vsseg_patch_acquisition` launch when a sample of the batch drew a family (`acquisition_launches` counts them).  `last_augment[b]` then also holds the fields
    of the sample's `vsseg_acquisition_job`: `thick`, `thick_offset`, `ghost_axis`, `ghosts`, `ghost_alpha` (fp32), `spike_amp` (fp32), `spike_k`, `spike_phase` (fp32).
    The scratch of the launch belongs to the sampler; nothing reads device memory or synchronises.  With the three ranges 0, or `acquisition_prob` 0, the sampler takes
    the paths above, launch for launch."""

    def __init__(self, cases: List[Dict], roi: Sequence[int], flip_prob: Optional[float] = 0.5, seed: Optional[int] = 0, *ranges, **named):
        self.cases, self.roi = cases, tuple(int(r) for r in roi)
        self.tail = RandomTail(self.roi, flip_prob, seed, Augmentation.of(*ranges, **named))
        self.appearing = self.tail.appearing and self.tail.appearance["appearance_prob"] > 0.0
        self.acquiring = self.tail.acquiring and self.tail.acquisition["acquisition_prob"] > 0.0
        self.acquisition_launches = 0
        self._acquisition_scratch: Optional[torch.Tensor] = None  # [B, *roi] of the largest batch so far: a job with thick slices and a later stage passes T(v) through it
        self.last_tone_stats: Optional[torch.Tensor] = None
        self._filter_scratch: Optional[torch.Tensor] = None  # [B, *roi] of the largest batch so far: a job with blur and low resolution passes the blurred patch through it
        self._tone_work: Optional[torch.Tensor] = None  # [B, TONE_SHARDS, 3] fp64
        self.lib = L.lib()
        self.last_draws: List[Tuple[bool, Tuple[int, int, int]]] = []
        self.last_augment: List[Dict] = []  # per sample: m (fp32 3x4), gain, bias, noise_std (fp32), noise_stream, seed (+ elastic_mag, bias_log (fp32), spacing with a field)

    def __len__(self):
        return len(self.cases)

    @staticmethod
    def _stage(jobs, dev) -> torch.Tensor:  # the bytes of a ctypes job table on the device; the caller issues `record_stream` on them after the launch that reads them
        return torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)

    def _scratch(self, attr: str, shape: Tuple[int, ...], dtype: torch.dtype, dev) -> torch.Tensor:  # the sampler's buffer `attr`: that of the largest batch so far on this device
        t = getattr(self, attr)
        if t is None or t.shape[0] < shape[0] or t.device != dev:
            t = torch.empty(shape, dtype=dtype, device=dev)
            setattr(self, attr, t)
        return t

    def sample(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        img, lab = self._sample_affine(indices) if self.tail.augmenting or self.tail.fielding else self._sample_crop(indices)
        if self.acquiring:
            img = self._acquisition(img)
        return (self._appearance(img), lab) if self.appearing else (img, lab)

    def _acquisition(self, img: torch.Tensor) -> torch.Tensor:
        """thick slices -> ghosting -> spike on the image patches [B, 1, *roi] of the crop launch; draws one sample after the other."""
        B, dev, stream = img.shape[0], img.device, torch.cuda.current_stream()
        if not self.last_augment:  # the plain crop keeps no per-sample record of its own
            self.last_augment = [dict() for _ in range(B)]
        jobs = (L.AcquisitionJob * B)()
        any_on = staged = False
        for b in range(B):
            job = self.tail.draw_acquisition(self.roi)
            self.last_augment[b].update(job)
            j = jobs[b]
            j.thick, j.thick_offset, j.ghost_axis, j.ghosts, j.ghost_alpha = job["thick"], job["thick_offset"], job["ghost_axis"], job["ghosts"], float(job["ghost_alpha"])
            j.spike_amp, j.spike_k, j.spike_phase = float(job["spike_amp"]), (C.c_int32 * 2)(*job["spike_k"]), float(job["spike_phase"])
            later = j.ghosts != 0 or j.spike_amp != 0.0
            any_on, staged = any_on or later or j.thick != 1, staged or (later and j.thick != 1)
        if not any_on:
            return img
        scratch = self._scratch("_acquisition_scratch", (B, *self.roi), torch.float32, dev).data_ptr() if staged else None
        jbuf = self._stage(jobs, dev)
        out = torch.empty_like(img)
        L.check(self.lib.vsseg_patch_acquisition(jobs, jbuf.data_ptr(), B, img.data_ptr(), out.data_ptr(), scratch, L.i3(self.roi), stream.cuda_stream), "patch_acquisition")
        jbuf.record_stream(stream)
        self.acquisition_launches += 1
        return out

    def _appearance(self, img: torch.Tensor) -> torch.Tensor:
        """blur -> low resolution -> contrast -> gamma on the image patches [B, 1, *roi] of the crop launch; draws one sample after the other."""
        B, dev, stream = img.shape[0], img.device, torch.cuda.current_stream()
        if not self.last_augment:  # the plain crop keeps no per-sample record of its own
            self.last_augment = [dict() for _ in range(B)]
        fjobs, tjobs = (L.FilterJob * B)(), (L.ToneJob * B)()
        filtering = toning = both = False
        for b in range(B):
            sigma, f, c, g = self.tail.draw_appearance()
            taps, coarse = blur_taps(sigma), coarse_size(self.roi, f)
            self.last_augment[b].update(blur_sigma=float(sigma), blur_taps=taps, coarse=coarse, contrast=np.float32(c), gamma=np.float32(g))
            fjobs[b].radius, fjobs[b].taps, fjobs[b].coarse = max(len(taps) - 1, 0), (C.c_float * 6)(*taps.tolist()), (C.c_int32 * 2)(*coarse)
            tjobs[b].contrast, tjobs[b].gamma = float(np.float32(c)), float(np.float32(g))
            low = coarse != self.roi[:2]
            filtering, both = filtering or low or len(taps) > 0, both or (low and len(taps) > 0)
            toning = toning or tjobs[b].contrast != 1.0 or tjobs[b].gamma != 1.0
        if filtering:
            scratch = self._scratch("_filter_scratch", (B, *self.roi), torch.float32, dev).data_ptr() if both else None
            jbuf = self._stage(fjobs, dev)
            out = torch.empty_like(img)
            L.check(self.lib.vsseg_patch_filter(fjobs, jbuf.data_ptr(), B, img.data_ptr(), out.data_ptr(), scratch, L.i3(self.roi), stream.cuda_stream), "patch_filter")
            jbuf.record_stream(stream)
            img = out
        self.last_tone_stats = None
        if toning:
            work = self._scratch("_tone_work", (B, L.TONE_SHARDS, 3), torch.float64, dev)
            jbuf = self._stage(tjobs, dev)
            self.last_tone_stats = torch.empty((B, 4), dtype=torch.float32, device=dev)
            L.check(self.lib.vsseg_patch_tone(tjobs, jbuf.data_ptr(), B, img.data_ptr(), img[0].numel(), self.last_tone_stats.data_ptr(), work.data_ptr(), stream.cuda_stream), "patch_tone")
            jbuf.record_stream(stream)
        return img

    def _sample_crop(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.cases[indices[0]]["image"].device
        B = len(indices)
        jobs = (L.CropJob * (2 * B))()
        self.last_draws, self.last_augment = [], []
        for b, i in enumerate(indices):
            case = self.cases[i]
            shape = tuple(case["image"].shape)
            flip, start = self.tail.draw(shape)
            self.last_draws.append((flip, start))
            for k, key in enumerate(("image", "label")):
                j = jobs[b + k * B]  # dst = [image_0..image_{B-1} | label_0..label_{B-1}]
                j.src, j.sdims, j.origin, j.flip_x = case[key].data_ptr(), L.i3(shape), L.i3(start), int(flip)
        jbuf = self._stage(jobs, dev)
        out = torch.empty((2, B, 1, *self.roi), dtype=torch.float32, device=dev)
        L.check(self.lib.vsseg_crop_flip(jbuf.data_ptr(), 2 * B, out.data_ptr(), L.i3(self.roi), torch.cuda.current_stream().cuda_stream), "crop_flip")
        jbuf.record_stream(torch.cuda.current_stream())
        return out[0], out[1]

    def _sample_affine(self, indices: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.cases[indices[0]]["image"].device
        B = len(indices)
        fielding = self.tail.fielding  # one vsseg_crop_field launch instead of one vsseg_crop_affine launch
        jobs = ((L.FieldJob if fielding else L.AffineJob) * (2 * B))()
        spacing = field_launch_spacing(self.tail.field["field_spacing"])
        self.last_draws, self.last_augment = [], []
        seed = self.tail.draw_noise_seed() + (self.tail.draw_field_seed() << 32)
        for b, i in enumerate(indices):
            case = self.cases[i]
            shape = tuple(case["image"].shape)
            flip, start = self.tail.draw(shape)
            angle, scale, gain, bias = self.tail.draw_augment() if self.tail.augmenting else (0.0, 1.0, 1.0, 0.0)
            m = affine_matrix(self.roi, start, shape[0], flip, angle, scale)
            aug = dict(m=m, gain=np.float32(gain), bias=np.float32(bias), noise_std=np.float32(self.tail.augment["noise_std"]), noise_stream=b, seed=seed)
            if fielding:
                mag, blog = self.tail.draw_field()
                aug.update(elastic_mag=np.float32(mag), bias_log=np.float32(blog), spacing=spacing)
            self.last_draws.append((flip, start))
            self.last_augment.append(aug)
            for k, key in enumerate(("image", "label")):
                j = jobs[b + k * B]  # dst = [image_0..image_{B-1} | label_0..label_{B-1}]
                j.src, j.sdims, j.m, j.noise_stream = case[key].data_ptr(), L.i3(shape), (C.c_float * 12)(*m.ravel().tolist()), b
                if key == "image":
                    j.interp, j.gain, j.bias, j.noise_std = L.INTERP_TRILINEAR, float(aug["gain"]), float(aug["bias"]), float(aug["noise_std"])
                else:
                    j.interp, j.gain, j.bias, j.noise_std = L.INTERP_NEAREST, 1.0, 0.0, 0.0
                if fielding:  # the label follows the deformation and knows no bias field
                    j.elastic_mag, j.bias_log = float(aug["elastic_mag"]), float(aug["bias_log"]) if key == "image" else 0.0
        jbuf = self._stage(jobs, dev)
        out = torch.empty((2, B, 1, *self.roi), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        if fielding:
            L.check(self.lib.vsseg_crop_field(jobs, jbuf.data_ptr(), 2 * B, out.data_ptr(), L.i3(self.roi), L.i3(spacing), seed, stream), "crop_field")
        else:
            L.check(self.lib.vsseg_crop_affine(jobs, jbuf.data_ptr(), 2 * B, out.data_ptr(), L.i3(self.roi), seed, stream), "crop_affine")
        jbuf.record_stream(torch.cuda.current_stream())
        return out[0], out[1]


def epoch_batches(n: int, batch_size: int, shuffle: bool, rng: np.random.RandomState, rank: int = 0, world: int = 1, pad: bool = True) -> List[List[int]]:
    """Index batches of one epoch: DataLoader(shuffle=True) order (ref:params/VSparams.py:311-318), sharded over ranks
    (rank r takes positions r, r+world, … of the shuffled list — SURVEY §8e) and cut into batches (last one may be short).

    `pad=True` (TRAINING loaders only): every rank gets the SAME number of indices, hence of batches — when n is not a multiple of
    `world` the list is padded by wrapping around to its own beginning (torch's DistributedSampler(drop_last=False) rule), because each
    training step issues a gradient all-reduce and unequal step counts would pair mismatched collectives.  Validation and test loaders
    pass `pad=False`: they issue ONE collective after their loop, so ranks may run different numbers of cases, and a wrapped case would
    be counted twice in the all-reduced Dice / loss sums (rank r then owns exactly `shard_indices(n, r, world)`)."""
    order = rng.permutation(n) if shuffle else np.arange(n)
    if pad and world > 1 and n % world and n > 0:
        pad = world - n % world
        order = np.concatenate([order, np.resize(order, pad)])
    mine = [int(i) for i in order[rank::world]]
    return [mine[i : i + batch_size] for i in range(0, len(mine), batch_size)]
