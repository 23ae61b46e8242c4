"""CPU tests of the path of the training augmentation from flag to launch: what tests/golden/make_augmentation_replay.py recorded from commit 2a48986
(tests/golden/augmentation_replay.json: every library call of PatchSampler with every field of every job, `last_draws`, `last_augment`, what VSparams makes of the 17
--aug_* flags, the parser's actions and the texts parser.error got) comes out exactly, and the one table of families (data.transforms.FAMILIES) is what the constructors,
the validators and the seeding go by."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from vs_seg_amd.data import transforms as T

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_augmentation_replay", os.path.join(HERE, "golden", "make_augmentation_replay.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

ON = (G.AUG, G.FIELD, dict(G.APP, appearance_prob=1.0), dict(G.ACQ, acquisition_prob=1.0))  # per family of the table, in its order
ZEROS = dict(elastic_mag=0.0, bias_field=0.0, field_spacing=16, blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, appearance_prob=1.0, thick_slices=0, ghost=0.0, spike=0.0, acquisition_prob=1.0)


@pytest.fixture(scope="module")
def recorded():
    with open(G.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    return G.record()


def test_the_recording_holds_the_configurations_it_should(recorded):
    names = [s["name"] for s in recorded["samplers"]]
    assert len(set(names)) == len(names) and {"off", "validation", "zeros given", "all four, p=0.0", "all four, p=0.5", "all four, p=1.0"} <= set(names)
    assert {k + " alone" for fam in T.FAMILIES for k in fam.ranges} <= set(names) and sum(n.startswith(fam.name + " alone") for fam in T.FAMILIES for n in names) == 4
    assert len({s["seed"] for s in recorded["samplers"]}) == 2 and all(len(s["batches"]) == 3 and len(b["last_draws"]) == 2 for s in recorded["samplers"] for b in s["batches"])
    launched = lambda name: [[c[0] for c in b["calls"]] for s in recorded["samplers"] if s["name"] == name for b in s["batches"]]  # noqa: E731
    assert launched("off") == [["vsseg_crop_flip"]] * 3
    assert launched("all four, p=1.0") == [["vsseg_crop_field", "vsseg_patch_acquisition", "vsseg_patch_filter", "vsseg_patch_tone"]] * 3
    assert launched("all four, p=0.0") == [["vsseg_crop_field"]] * 3
    assert all(c[1 + recorded["call_args"][c[0]].index("jobs_dev")] == "= jobs" for s in recorded["samplers"] for b in s["batches"] for c in b["calls"] if c[0] != "vsseg_crop_flip")
    assert len(recorded["params"]) >= 19 and len(recorded["rejected"]) >= 12 and len(recorded["flags"]["aug"]) == 17
    assert os.path.getsize(G.PATH) < os.path.getsize(os.path.join(HERE, "golden", "inference_reports.json"))


def test_the_sampler_hands_the_library_what_the_parent_did(recorded, replayed):
    assert replayed["job_fields"] == recorded["job_fields"] and replayed["call_args"] == recorded["call_args"]  # the structures and entry points themselves did not move
    assert [s["name"] for s in replayed["samplers"]] == [s["name"] for s in recorded["samplers"]]
    for got, want in zip(replayed["samplers"], recorded["samplers"]):
        assert got.keys() == want.keys()
        for k in want:
            if k != "batches":
                assert got[k] == want[k], (want["name"], k)
        for i, (gb, wb) in enumerate(zip(got["batches"], want["batches"])):
            for k in wb:  # calls, last_draws, last_augment, acquisition_launches, last_tone_stats, image
                assert gb[k] == wb[k], (want["name"], i, k)
        assert len(got["batches"]) == len(want["batches"])


def test_vsparams_makes_of_the_flags_what_the_parent_did(recorded, replayed):
    assert len(replayed["params"]) == len(recorded["params"])
    for got, want in zip(replayed["params"], recorded["params"]):
        assert got.keys() == want.keys()
        for k in want:  # argv, train, val, test, attributes, properties
            assert got[k] == want[k], (want["argv"], k)
        assert set(want["train"]) - set(want["val"]) == {fam.key for fam in T.FAMILIES} and set(want["val"]) == set(want["test"])  # the four keys on the training dict only


def test_the_flags_and_the_rejections_are_the_parents(recorded, replayed):
    assert replayed["flags"]["order"] == recorded["flags"]["order"]
    for got, want in zip(replayed["flags"]["aug"], recorded["flags"]["aug"]):
        assert got == want, want["option_strings"]
    assert replayed["rejected"] == recorded["rejected"]


def test_the_generator_writes_the_file_byte_for_byte(replayed):
    with open(G.PATH) as f:
        assert G.dumps(replayed) == f.read()


def test_the_stand_in_leaves_nothing_behind(replayed):
    from vs_seg_amd import _lib as L

    assert L.lib.__name__ == "lib" and torch.Tensor.record_stream.__name__ == "record_stream" and torch.cuda.current_stream.__module__.startswith("torch")


# ---- the table ----
def test_keys_and_validators_are_views_of_the_table():
    assert [fam.key for fam in T.FAMILIES] == ["augment", "field_augment", "appearance_augment", "acquisition_augment"]
    assert [fam.rng for fam in T.FAMILIES] == ["_augR", "_fieldR", "_appR", "_acqR"]
    assert (T.AUGMENT_KEYS, T.FIELD_KEYS, T.APPEARANCE_KEYS, T.ACQUISITION_KEYS) == tuple(tuple(fam.defaults) for fam in T.FAMILIES)
    assert T.AUGMENT_KEYS == ("rotate_deg", "scale", "intensity_scale", "intensity_shift", "noise_std") and T.FIELD_KEYS == ("elastic_mag", "bias_field", "field_spacing")
    assert T.APPEARANCE_KEYS == ("blur_sigma", "lowres", "contrast", "gamma", "appearance_prob") and T.ACQUISITION_KEYS == ("thick_slices", "ghost", "spike", "acquisition_prob")
    assert all(set(fam.ranges) < set(fam.defaults) or fam.name == "augment" for fam in T.FAMILIES) and not {"field_spacing", "appearance_prob", "acquisition_prob"} & {k for fam in T.FAMILIES for k in fam.ranges}
    for check, fam in zip((T.check_augment, T.check_field_augment, T.check_appearance_augment, T.check_acquisition_augment), T.FAMILIES):
        assert check() == fam.defaults and list(check()) == list(fam.defaults) and check == fam.check
    f = T.check_field_augment(2, bias_field="0.25", field_spacing=16.0)
    assert f == dict(elastic_mag=2.0, bias_field=0.25, field_spacing=16) and [type(v) for v in f.values()] == [float, float, int]
    q = T.check_acquisition_augment(3.0, 1, acquisition_prob=1)
    assert q == dict(thick_slices=3, ghost=1.0, spike=0.0, acquisition_prob=1.0) and [type(v) for v in q.values()] == [int, float, float, float]
    for check, bad, text in ((T.check_augment, dict(scale=-0.5), "augmentation range scale = -0.5: must be finite and >= 0"), (T.check_field_augment, dict(bias_field=float("nan")), "augmentation range bias_field = nan: must be finite and >= 0"),
                             (T.check_appearance_augment, dict(appearance_prob=-1), "augmentation range appearance_prob = -1.0: must be finite and >= 0"),
                             (T.check_acquisition_augment, dict(thick_slices=-2), "augmentation range thick_slices = -2.0: must be finite and >= 0"),
                             (T.check_field_augment, dict(elastic_mag=-1, field_spacing=0), "augmentation range elastic_mag = -1.0: must be finite and >= 0"),  # the shared rule comes first
                             (T.check_acquisition_augment, dict(thick_slices="2.5"), "thick_slices = 2.5: 0 (off) or an integer slab height in 2..4 voxels")):
        with pytest.raises(ValueError) as e:
            check(**bad)
        assert str(e.value) == text
    with pytest.raises(TypeError):
        T.check_augment(0, 0, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        T.check_augment(0.0, rotate_deg=1.0)
    with pytest.raises(TypeError):
        T.check_field_augment(gamma=0.1)


def test_the_record_binds_like_a_call():
    a = T.Augmentation.of(10.0, 0.1, field_spacing=32, gamma=0.5, thick_slices=2.0)
    assert a.values["augment"] == dict(rotate_deg=10.0, scale=0.1, intensity_scale=0.0, intensity_shift=0.0, noise_std=0.0) and a.values["field"]["field_spacing"] == 32
    assert [a.on(fam) for fam in T.FAMILIES] == [True, False, True, True] and T.Augmentation.of(a) is a
    assert list(a.flat()) == [k for fam in T.FAMILIES for k in fam.defaults] and a.flat()["thick_slices"] == 2 and type(a.flat()["thick_slices"]) is int
    assert [T.Augmentation.of(field_spacing=8, appearance_prob=1.0, acquisition_prob=0.0).on(fam) for fam in T.FAMILIES] == [False] * 4  # no range, nothing on
    with pytest.raises(ValueError, match="rotate_deg = 181.0: at most 180"):
        T.Augmentation.of(181.0, blur_sigma=9.0)  # the first family of the table that objects


def _tails(make):
    """The same settings by five positional zeros, by names and by a mixture; then all four families on, by names and by a mixture."""
    zeros = [make(0.0, 0.0, 0.0, 0.0, 0.0), make(**dict.fromkeys(T.AUGMENT_KEYS, 0.0), **ZEROS), make(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 16, **{k: v for k, v in ZEROS.items() if k not in T.FIELD_KEYS}), make()]
    every = {k: v for d in ON for k, v in d.items()}
    on = [make(**every), make(*every.values()), make(*G.AUG.values(), *G.FIELD.values(), **ON[2], **ON[3])]
    return zeros, on


def test_call_forms_of_random_tail():
    zeros, on = _tails(lambda *r, **n: T.RandomTail((8, 8, 4), 0.5, 3, *r, **n))
    for tails in ((zeros[0], zeros[3]), (zeros[1], zeros[2]), on, zeros):  # (five zeros leave the defaults, which differ from ZEROS in what is no range)
        for fam in T.FAMILIES:
            assert all(getattr(t, fam.flag) == getattr(tails[0], fam.flag) and (tails is zeros or getattr(t, fam.name) == getattr(tails[0], fam.name)) for t in tails)
        draws = [[t.draw((12, 11, 6)) for _ in range(4)] for t in tails]
        assert all(d == draws[0] for d in draws)
    assert not any(getattr(zeros[0], fam.flag) or getattr(zeros[0], fam.rng) is not None for fam in T.FAMILIES)
    assert all(getattr(on[0], fam.flag) and getattr(on[0], fam.name) == T.FAMILIES[i].check(**ON[i]) for i, fam in enumerate(T.FAMILIES))
    assert on[1].draw_augment() == on[0].draw_augment() and on[2].draw_acquisition() == on[0].draw_acquisition()


def test_call_forms_of_patch_sampler():
    with G.standin():
        cases = [dict(image=torch.zeros(12, 11, 6), label=torch.zeros(12, 11, 6))]
        zeros, on = _tails(lambda *r, **n: T.PatchSampler(cases, (8, 8, 4), 0.5, 3, *r, **n))
        assert not any(s.appearing or s.acquiring or s.tail.augmenting or s.tail.fielding for s in zeros)
        for s in on:
            s.sample([0, 0])
        for s in on[1:]:
            assert s.appearing and s.acquiring and s.tail.augmentation == on[0].tail.augmentation and s.last_draws == on[0].last_draws and s.acquisition_launches == 1
            assert all(np.array_equal(a[k], b[k]) for a, b in zip(s.last_augment, on[0].last_augment) for k in b) and len(s.last_augment) == 2
        by_record = T.PatchSampler(cases, (8, 8, 4), 0.5, 3, on[0].tail.augmentation)  # what CachedLoader hands on
        assert by_record.tail.augmentation is on[0].tail.augmentation and by_record.tail.acquisition == on[0].tail.acquisition


@pytest.mark.parametrize("make", [lambda *r, **n: T.RandomTail((8, 8, 4), 0.5, 3, *r, **n), lambda *r, **n: T.PatchSampler([], (8, 8, 4), 0.5, 3, *r, **n)], ids=["RandomTail", "PatchSampler"])
def test_unknown_and_doubled_names_are_type_errors(make):
    with G.standin():
        with pytest.raises(TypeError, match="unexpected keyword argument 'rotate'"):
            make(rotate=10.0)
        with pytest.raises(TypeError, match="multiple values for argument 'scale'"):
            make(10.0, 0.1, scale=0.2)
        with pytest.raises(TypeError, match="multiple values for argument 'field_spacing'"):
            make(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 16, field_spacing=16)
        with pytest.raises(TypeError):
            make(*([0.0] * 18))
        with pytest.raises(ValueError, match="thick_slices = 7"):
            make(thick_slices=7)


@pytest.mark.parametrize("flip_prob", [0.5, None])
def test_the_order_of_the_table_is_the_seeding_order(flip_prob):
    seed = 11
    for k, fam in enumerate(T.FAMILIES):  # family k alone: its state is seeded right after crop
        R = np.random.RandomState(seed)
        first = [np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32")) for _ in range(2 if flip_prob is not None else 1)]
        want = np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32"))
        tail = T.RandomTail((8, 8, 4), flip_prob, seed, **ON[k])
        assert [getattr(tail, f.flag) for f in T.FAMILIES] == [f is fam for f in T.FAMILIES] and [getattr(tail, f.rng) is None for f in T.FAMILIES] == [f is not fam for f in T.FAMILIES]
        assert getattr(tail, fam.rng).randint(1 << 30, size=4).tolist() == want.randint(1 << 30, size=4).tolist()
        assert tail._cropR.randint(1 << 30) == first[-1].randint(1 << 30) and (flip_prob is None) == (tail._flipR is None)
    R = np.random.RandomState(seed)  # all on: flip, crop, then the table from top to bottom
    seeds = [R.randint(T.MAX_SEED, dtype="uint32") for _ in range((2 if flip_prob is not None else 1) + len(T.FAMILIES))]
    tail = T.RandomTail((8, 8, 4), flip_prob, seed, **{k: v for d in ON for k, v in d.items()})
    for fam, s in zip(T.FAMILIES, seeds[-len(T.FAMILIES):]):
        assert getattr(tail, fam.rng).randint(1 << 30) == np.random.RandomState(s).randint(1 << 30), fam.name
    assert tail.set_random_state(seed) is tail and tail._acqR.randint(1 << 30) == np.random.RandomState(seeds[-1]).randint(1 << 30)  # re-seeding goes the same way


def test_cached_loader_takes_the_families_by_their_transform_keys():
    from vs_seg_amd import params as P

    with G.standin():
        cases = [dict(image=torch.zeros(12, 11, 6), label=torch.zeros(12, 11, 6), image_meta={}, label_meta={})]
        on = P.CachedLoader(cases, (8, 8, 4), 1, True, 0.5, seed=0, augment=G.AUG, field_augment=None, acquisition_augment=ON[3])
        t = on.sampler.tail
        assert (t.augmenting, t.fielding, t.appearing, t.acquiring) == (True, False, False, True) and t.augment == G.AUG and t.acquisition == ON[3] and t.field == T.check_field_augment()
        assert next(iter(on))["image"].shape == (1, 1, 8, 8, 4) and on.sampler.acquisition_launches == 1
        off = P.CachedLoader(cases, (8, 8, 4), 1, False, None)
        assert not any(getattr(off.sampler.tail, fam.flag) for fam in T.FAMILIES) and P.CachedLoader(cases, None, 1, False, None, augment=G.AUG).sampler is None
        with pytest.raises(TypeError, match="unexpected keyword argument 'augmentation'"):
            P.CachedLoader(cases, (8, 8, 4), 1, True, 0.5, augmentation=G.AUG)
