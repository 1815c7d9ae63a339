"""CPU checks of crop training (pytorch_camvid_amd.transforms.CropCompose and the cvk_crop_* entry points): the size rules on
hand-computed cases, the order and number of the `random` calls, the flipped-and-narrow and centred-pad offset rules, packed records,
argument validation without a launch, refused pipelines, the selection rule of the restatement (tests/crop_aug_ref.py) on crafted
count tables, and the condition under which the GPU tests' rounding bands cannot hide a wrong kernel."""
import ctypes
import random

import numpy as np
import pytest

from pytorch_camvid_amd import _lib
from pytorch_camvid_amd import transforms as T

from tests import crop_aug_ref as C

MEAN = (0.42019099703461577, 0.41323568513979647, 0.4010048431259079)
STD = (0.30598050258519743, 0.3089986932156864, 0.3054061869915674)


def test_resized_hw_on_hand_computed_cases():
    assert T.resized_hw(720, 960, 1.0, scale=(2048, 512)) == (512, 683)       # sf = min(2048/960, 512/720) = 0.7111: 682.67 -> 683
    assert T.resized_hw(720, 960, 0.5) == (360, 480) and T.resized_hw(720, 960, 2.0) == (1440, 1920)
    assert T.resized_hw(45, 83, 0.5) == (23, 42)                              # 22.5 -> 23 (half up), 41.5 -> 42
    assert T.resized_hw(45, 83, 0.61) == (27, 51)                             # 27.45, 50.63
    # keep-ratio at both ends: L = 1024, S = 256 -> sf = min(1024/960, 256/720) = 0.3556; L = 4096, S = 1024 -> sf = 1.4222
    assert T.resized_hw(720, 960, 0.5, scale=(2048, 512)) == (256, 341)
    assert T.resized_hw(720, 960, 2.0, scale=(512, 2048)) == (1024, 1365)
    assert T.resized_hw(3, 400, 0.1) == (1, 40)                               # 0.3 would round to 0
    assert T.resized_hw(2, 960, 0.5, scale=(100, 20)) == (1, 50)              # sf = min(50/960, 10/2): 0.104 rows -> 1


def _crop_pipe(**kw):
    return T.crop_transforms(crop_size=(33, 70), **kw)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_seeded_draw_makes_the_stated_random_calls_in_the_stated_order(seed):
    Hs, Ws = 45, 83
    pipe = _crop_pipe(blur=True)
    random.seed(seed)
    drawn = [pipe.draw(Hs, Ws) for _ in range(6)]
    after = random.getstate()
    random.seed(seed)
    for p in drawn:                                                           # the same calls by hand
        r = random.uniform(0.5, 2.0)
        Hr, Wr = T.resized_hw(Hs, Ws, r)
        cands = []
        for _ in range(11):
            oy = random.randint(0, max(Hr - 33, 0))
            cands.append((oy, random.randint(0, max(Wr - 70, 0))))
        blur = None
        if random.random() < 0.5:
            sigma = random.uniform(0.0, 3.0)
            blur = (T.RandomGaussianBlur._compute_gaussian_blur_ksize(sigma), sigma)
        flip = random.random() < 0.5
        jitter = None
        if not random.random() < 0.4:
            jitter = [("brightness", random.uniform(0.6, 1.4))]
            random.shuffle(jitter)
        if flip and Wr < 70:
            cands = [(oy, Wr - 70) for oy, _ in cands]
        assert (p["r"], p["Hr"], p["Wr"], p["sy"], p["sx"]) == (r, Hr, Wr, Hs / Hr, Ws / Wr)
        assert p["cands"] == cands and p["blur"] == blur and p["flip"] == flip and p["jitter"] == jitter
    assert random.getstate() == after
    # cat_max_ratio = 1 tests nothing: one pair
    one = _crop_pipe(cat_max_ratio=1.0, jitter=False)
    random.seed(seed)
    p = one.draw(Hs, Ws)
    after = random.getstate()
    random.seed(seed)
    Hr, Wr = T.resized_hw(Hs, Ws, random.uniform(0.5, 2.0))
    oy = random.randint(0, max(Hr - 33, 0)); ox = random.randint(0, max(Wr - 70, 0))
    flip = random.random() < 0.5
    assert len(p["cands"]) == 1 and p["cands"][0] == (oy, Wr - 70 if flip and Wr < 70 else ox) and random.getstate() == after


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scale_jitter_draws_and_centred_offsets(seed):
    Hs, Ws = 45, 83
    pipe = T.CropCompose([T.ScaleJitter((0.5, 2.0), value=11), T.RandomHorizontalFlip(), T.ToTensor(), T.Normalize(MEAN, STD)])
    assert pipe.out_hw(Hs, Ws) == (Hs, Ws) and pipe.pad_normalized == 1 and pipe.pad_label == 11 and pipe.cat_max_ratio == 1.0
    random.seed(seed)
    drawn = [pipe.draw(Hs, Ws) for _ in range(6)]
    after = random.getstate()
    random.seed(seed)
    for p in drawn:
        s = random.uniform(0.5, 2.0)
        Hr, Wr = round(s * Hs), round(s * Ws)
        h, w = max(Hr, Hs), max(Wr, Ws)                                       # the padded size
        y1 = random.randint(0, h - Hs); x1 = random.randint(0, w - Ws)
        flip = random.random() < 0.5
        assert (p["Hr"], p["Wr"], p["sy"], p["sx"], p["flip"]) == (Hr, Wr, 1 / s, 1 / s, flip)
        assert p["cands"] == [(y1 - max(0, Hs - Hr) // 2, x1 - max(0, Ws - Wr) // 2)]
    assert random.getstate() == after


def test_scale_jitter_hand_computed_offsets(monkeypatch):
    pipe = T.CropCompose([T.ScaleJitter(), T.ToTensor()])
    monkeypatch.setattr(random, "uniform", lambda a, b: 0.5)
    calls = []
    monkeypatch.setattr(random, "randint", lambda a, b: calls.append((a, b)) or b)
    p = pipe.draw(45, 83)
    # round(22.5) = 22 and round(41.5) = 42 (half to even); diff 23, 41 -> 11 rows on top, 20 columns on the left; no room to move
    assert (p["Hr"], p["Wr"]) == (22, 42) and p["cands"] == [(-11, -20)] and calls == [(0, 0), (0, 0)] and p["sy"] == 2.0
    monkeypatch.setattr(random, "uniform", lambda a, b: 2.0)
    calls.clear()
    p = pipe.draw(45, 83)
    assert (p["Hr"], p["Wr"]) == (90, 166) and calls == [(0, 45), (0, 83)] and p["cands"] == [(45, 83)] and p["sx"] == 0.5
    monkeypatch.setattr(random, "uniform", lambda a, b: 0.001)
    assert pipe.draw(45, 83)["Hr"] == 1                                       # would round to 0


def test_flipped_and_narrow_samples_keep_their_content_at_the_left(monkeypatch):
    pipe = T.CropCompose([T.RandomResize((0.5, 0.5)), T.RandomCrop((33, 70)), T.RandomHorizontalFlip(p=1.0), T.ToTensor()])
    random.seed(0)
    p = pipe.draw(45, 83)                                                     # 23 x 42: narrower and lower than the crop
    assert p["flip"] and (p["Hr"], p["Wr"]) == (23, 42) and len(p["cands"]) == 11
    assert all(c == (0, 42 - 70) for c in p["cands"])                         # pad bottom stays, pad moves to the canvas' left
    never = T.CropCompose([T.RandomResize((0.5, 0.5)), T.RandomCrop((33, 70)), T.RandomHorizontalFlip(p=0.0), T.ToTensor()])
    assert all(c == (0, 0) for c in never.draw(45, 83)["cands"])
    wide = T.CropCompose([T.RandomResize((2.0, 2.0)), T.RandomCrop((33, 70)), T.RandomHorizontalFlip(p=1.0), T.ToTensor()])
    p = wide.draw(45, 83)
    assert all(0 <= oy <= 90 - 33 and 0 <= ox <= 166 - 70 for oy, ox in p["cands"]) and len(set(p["cands"])) > 1


def test_pack_round_trips_and_the_record_size():
    assert T.CROP_RECORD.itemsize == ctypes.sizeof(_lib.CropRecord) == _lib.load().cvk_crop_record_bytes() == 416
    params = [{"r": 0.5, "Hr": 23, "Wr": 42, "sy": 45 / 23, "sx": 83 / 42, "cands": [(0, -28)] * 11, "flip": True, "blur": (9, 2.9),
               "jitter": [("brightness", 1.3)]},
              {"r": 2.0, "Hr": 90, "Wr": 166, "sy": 0.5, "sx": 0.5, "cands": [(5, 7), (-3, 96)], "flip": False, "blur": None, "jitter": None}]
    rec = T.CropCompose.pack(params)
    assert rec["Hr"].tolist() == [23, 90] and rec["Wr"].tolist() == [42, 166] and rec["ncand"].tolist() == [11, 2]
    assert rec["sy"].tolist() == [45 / 23, 0.5] and rec["sx"].tolist() == [83 / 42, 0.5]
    assert rec[0]["offy"].tolist() == [0] * 11 and rec[0]["offx"].tolist() == [-28] * 11
    assert rec[1]["offy"].tolist() == [5, -3] + [0] * 9 and rec[1]["offx"].tolist() == [7, 96] + [0] * 9
    assert rec["flip"].tolist() == [1, 0] and rec["ksize"].tolist() == [9, 0] and rec["use_lut"].tolist() == [1, 0]
    assert np.array_equal(rec[0]["taps"], T.gaussian_taps(9, 2.9).astype(np.float32)) and (rec[1]["taps"] == 0).all()
    assert np.array_equal(rec[0]["lut"], T.brightness_lut(1.3))
    out = np.full(2, 255, dtype=np.uint8).repeat(416).view(T.CROP_RECORD)       # `out` is cleared, then filled
    assert T.CropCompose.pack(params, out=out) is out and out.tobytes() == rec.tobytes()
    with pytest.raises(ValueError):
        T.CropCompose.pack([dict(params[0], cands=[(0, 0)] * 12)])
    # field offsets of include/cvk.h
    assert [T.CROP_RECORD.fields[k][1] for k in ("sy", "Hr", "ncand", "offy", "offx", "taps", "flip", "ksize", "lut")] == \
        [0, 16, 24, 28, 72, 116, 152, 154, 160]


def test_crop_entry_points_validate_their_arguments_without_gpu():
    lib = _lib.load()
    m = (ctypes.c_float * 3)(*MEAN)
    sd = (ctypes.c_float * 3)(*STD)
    z = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    p = 4096                                         # a fake, 16-byte aligned device address: every call below is refused first

    def sel(masks=p, mb=1, N=2, Hs=45, Ws=83, hc=33, wc=70, rec=p, ratio=0.75, counts=p, selection=p):
        return lib.cvk_crop_select(masks, mb, N, Hs, Ws, hc, wc, rec, 11, ratio, counts, selection, None)

    for kw in (dict(masks=None), dict(rec=None), dict(counts=None), dict(selection=None)):
        assert sel(**kw) == -1 and b"null" in lib.cvk_last_error_string(), kw
    for kw in (dict(mb=4), dict(N=0), dict(Hs=0), dict(Ws=-1), dict(hc=0), dict(wc=0)):
        assert sel(**kw) == -1 and b"bad arguments" in lib.cvk_last_error_string(), kw
    for ratio in (0.0, -0.5, 1.0000001, float("nan")):
        assert sel(ratio=ratio) == -1 and b"cat_max_ratio" in lib.cvk_last_error_string(), ratio
    for kw in (dict(N=70000), dict(hc=50000, wc=50000)):
        assert sel(**kw) == -1 and b"grid" in lib.cvk_last_error_string(), kw

    def aug(frames=p, masks=p, mb=1, N=2, Hs=45, Ws=83, hc=33, wc=70, rec=p, selection=p, mean=m, std=sd, out=p, om=p):
        return lib.cvk_crop_augment_u8(frames, masks, mb, N, Hs, Ws, hc, wc, rec, selection, mean, std, 11, 0, out, om, None, None)

    for kw in (dict(frames=None), dict(masks=None), dict(rec=None), dict(selection=None), dict(mean=None), dict(std=None), dict(out=None),
               dict(om=None)):
        assert aug(**kw) == -1 and b"null" in lib.cvk_last_error_string(), kw
    for kw in (dict(mb=2), dict(N=0), dict(Hs=0), dict(Ws=0), dict(hc=-3), dict(wc=0), dict(out=p + 4)):
        assert aug(**kw) == -1 and b"bad arguments" in lib.cvk_last_error_string(), kw
    for kw in (dict(N=70000), dict(hc=16 * 65536)):
        assert aug(**kw) == -1 and b"grid" in lib.cvk_last_error_string(), kw
    assert aug(std=z) == -1 and b"zero std" in lib.cvk_last_error_string()


def test_refused_and_accepted_pipelines():
    tail = [T.RandomHorizontalFlip(), T.ToTensor(), T.Normalize(MEAN, STD)]
    rr, rc = T.RandomResize(), T.RandomCrop((33, 70))
    T.CropCompose([rr, rc] + tail)
    T.CropCompose([rr, rc, T.RandomGaussianBlur(), T.RandomHorizontalFlip(), T.ColorJitter(0.4, 0.4), T.ToTensor(), T.Normalize(MEAN, STD)])
    T.CropCompose([T.ScaleJitter()] + tail)
    for bad in ([rc, rr] + tail, [rr] + tail, [rc] + tail, tail, [rr, rc, T.Resize((70, 33))] + tail, [T.Resize((70, 33)), rr, rc] + tail,
                [rr, rc, T.RandomRotation(15)] + tail, [rr, rc, T.RandomHorizontalFlip(), T.RandomGaussianBlur(), T.ToTensor()],
                [rr, rc, T.RandomHorizontalFlip(), T.Normalize(MEAN, STD)], [T.ScaleJitter(), rc] + tail, [rr, rc, rr, rc] + tail,
                [rr, rc, T.ToTensor(), T.RandomHorizontalFlip()]):
        with pytest.raises(NotImplementedError):
            T.CropCompose(bad)
    with pytest.raises(NotImplementedError):
        T.Compose([rr, rc] + tail)                                            # the fixed pipeline's Compose is what it was
    with pytest.raises(NotImplementedError):
        T.RandomScale()
    with pytest.raises(NotImplementedError):
        T.ColorJitter(0.4, 0.4, 0.0, 0.4)
    for bad in (lambda: T.RandomCrop((33, 70), cat_max_ratio=0.0), lambda: T.RandomCrop((33, 70), cat_max_ratio=1.5),
                lambda: T.RandomCrop((0, 70)), lambda: T.RandomResize((0.0, 1.0)), lambda: T.RandomResize((2.0, 1.0)),
                lambda: T.ScaleJitter((0.0, 2.0))):
        with pytest.raises(ValueError):
            bad()
    c = T.crop_transforms()
    assert c.out_hw(720, 960) == (360, 480) and c.mean == MEAN and c.std == STD and c.last_selection is None
    assert c.pad_label == 11 and c.pad_normalized == 0 and c.cat_max_ratio == 0.75 and c.ignore_index == 11
    assert [type(t).__name__ for t in c.transforms] == ["RandomResize", "RandomCrop", "RandomHorizontalFlip", "ColorJitter", "ToTensor",
                                                        "Normalize"]
    assert "RandomGaussianBlur" in repr(T.crop_transforms(blur=True)) and "ColorJitter" not in repr(T.crop_transforms(jitter=False))


def _table(rows):
    t = np.zeros((11, 256), dtype=np.uint32)
    for c, row in enumerate(rows):
        for label, n in row.items():
            t[c, label] = n
    return t


def test_selection_rule_of_the_restatement_on_crafted_tables():
    one, mixed, heavy = {3: 1000}, {3: 700, 5: 300}, {3: 900, 5: 100}
    assert C.select(_table([mixed] + [one] * 10), 11, 0.75) == (0, 1)
    assert C.select(_table([one, heavy, mixed, mixed] + [one] * 7), 11, 0.75) == (2, 1)     # the first that passes
    assert C.select(_table([one, heavy] * 5 + [mixed]), 11, 0.75) == (10, 0)                 # the fallback is not tested
    assert C.select(_table([one] * 11), 11, 0.75) == (10, 0)                                 # a single class never passes
    assert C.select(_table([{}] * 11), 11, 0.75) == (10, 0)                                  # nothing counted (all void / all pad)
    assert C.select(_table([{3: 750, 5: 250}, {3: 749, 5: 251}]), 3, 0.75) == (1, 1)         # exactly the ratio fails
    assert C.select(_table([{3: 3, 5: 1}]), 2, 0.75) == (1, 0)
    assert C.select(_table([mixed]), 1, 1.0) == (0, 0)                                       # ncand = 1 tests nothing
    assert C.select(_table([one, mixed]), 2, 1.0) == (1, 0)
    # counts come from labels: void (ignore_index) and labels outside [0, 256) are excluded before the rule sees them
    mask = np.full((40, 40), 11, dtype=np.int64)
    mask[:10] = 3
    mask[10:12] = 4000
    mask[12:14] = -1
    cnt = C.candidate_counts(mask, 40, 40, 1.0, 1.0, 40, 40, 0, 0, 11)
    assert cnt[3] == 400 and cnt.sum() == 400
    assert C.select(np.stack([cnt] * 2), 2, 0.75) == (1, 0)                                  # one class + void is one class
    # pad is not counted: the window hangs over the bottom-right corner
    cnt = C.candidate_counts(np.full((40, 40), 2, dtype=np.uint8), 40, 40, 1.0, 1.0, 30, 30, 25, 20, 11)
    assert cnt[2] == 15 * 20 and cnt.sum() == 300
    cnt = C.candidate_counts(np.full((40, 40), 2, dtype=np.uint8), 20, 20, 2.0, 2.0, 30, 30, -15, -15, 11)
    assert cnt[2] == 15 * 15


def test_share_of_values_inside_the_rounding_bands_is_at_most_one_percent():
    """The GPU tests let the kernel differ from the restatement only where the fp64 value lies within a derived delta of a
    half-integer.  For their inputs that is at most 1 % of the values, so the band cannot hide a wrong kernel."""
    frames, _ = C.frames_masks()
    assert 2.0 ** -12 < C.DELTA_RESIZE < 2.0 ** -11
    for name, Hr, Wr, sy, sx in C.step_cases():
        for n in range(C.N):
            pre = C.resize_linear_pre(frames[n], Hr, Wr, sy, sx)
            assert C.near_half(pre, C.DELTA_RESIZE).mean() <= 0.01, (name, n)
            u8 = C.round_u8(pre)
            for k, sigma in C.BLURS:
                taps = T.gaussian_taps(k, sigma).astype(np.float32).astype(np.float64)
                assert C.near_half(C.blur_pre(u8, taps), C.blur_delta(k)).mean() <= 0.01, (name, n, k)


def test_restatement_agrees_with_the_fixed_pipeline_restatement():
    """with steps Hs / H, zero offsets and the crop equal to the resized size it is tests/augment_ref.py's augment"""
    from tests import augment_ref as R
    frames, masks = C.frames_masks()
    taps = T.gaussian_taps(5, 1.3)
    for H, W in ((33, 70), (60, 101)):
        a = R.augment(frames[0], masks[0], H, W, 5, taps, True, T.brightness_lut(1.2))
        x, m, inside = C.crop_augment(frames[0], masks[0], H, W, 45 / H, 83 / W, H, W, 0, 0, 5, taps, True, T.brightness_lut(1.2))
        assert inside.all() and np.array_equal(a[0], x) and np.array_equal(a[1], m)
