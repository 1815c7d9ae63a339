"""Crop training on the device (cvk_crop_select + cvk_crop_augment_u8 via pytorch_camvid_amd.transforms) against the fp64 restatement
in tests/crop_aug_ref.py.  Exact: the count and selection tables, masks, pad, flip, LUT, normalisation, and image values under dyadic
steps.  Other steps and the blur may differ by one level only where the fp64 value lies within a derived delta of a half-integer
(tests/crop_aug_ref.py derives the deltas; tests/test_crop_aug_cpu.py asserts that at most 1 % of the values lie there)."""
import random

import numpy as np
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import transforms as T

from tests import crop_aug_ref as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, HS, WS, HC, WC = C.N, C.HS, C.WS, C.HC, C.WC
VOID = 11


def _p(Hr, Wr, sy, sx, cands, flip=False, blur=None, jitter=None):
    return {"r": None, "Hr": Hr, "Wr": Wr, "sy": sy, "sx": sx, "cands": list(cands), "flip": flip, "blur": blur, "jitter": jitter}


def _run(frames, masks, params, hc=HC, wc=WC, ratio=0.75, pad_label=VOID, pad_normalized=0, mask_dtype=torch.uint8):
    """-> x, m, u8 (device), counts uint32 [N,11,256], selection int32 [N,4] (host), records (numpy)"""
    rec = T.CropCompose.pack(params)
    n = len(params)
    grec = torch.from_numpy(rec.view(np.uint8)).to(DEV)
    gf, gm = torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV).to(mask_dtype)
    counts = torch.full((n, 11, 256), -1, device=DEV, dtype=torch.int32)              # the call clears it
    sel = torch.full((n, 4), -77, device=DEV, dtype=torch.int32)
    T.crop_select(gm, grec, frames.shape[1:3], (hc, wc), VOID, ratio, counts, sel)
    x, m, u8 = T.crop_augment_u8(gf, gm, grec, sel, (hc, wc), pad_label=pad_label, pad_normalized=pad_normalized, out_u8=True)
    torch.cuda.synchronize()
    return x, m, u8, counts.cpu().numpy().view(np.uint32), sel.cpu().numpy(), rec


def _ref(frames, masks, rec, sel, hc=HC, wc=WC, pad_label=VOID):
    out = []
    for i, r in enumerate(rec):
        k = int(r["ksize"])
        out.append(C.crop_augment(frames[i], masks[i], int(r["Hr"]), int(r["Wr"]), float(r["sy"]), float(r["sx"]), hc, wc,
                                  int(sel[i][1]), int(sel[i][2]), k, r["taps"].astype(np.float64), bool(r["flip"]),
                                  r["lut"] if r["use_lut"] else None, pad_label))
    return out


def _band(pre_near, r, sel_row, hc=HC, wc=WC):
    """the [Hr,Wr,3] band mask seen through the window and the flip"""
    b, _ = C.window(pre_near, hc, wc, int(sel_row[1]), int(sel_row[2]), False)
    return b[:, ::-1] if r["flip"] else b


def _check_values(got, want, band, r, tag):
    """equal outside the band; inside it one level, or the LUT's largest step where a LUT was applied"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d[~band].max(initial=0) == 0, (tag, int((d[~band] > 0).sum()), int(d[~band].max()))
    allowed = max(1, int(np.abs(np.diff(r["lut"].astype(np.int32))).max())) if r["use_lut"] else 1
    assert d.max(initial=0) <= allowed, (tag, int(d.max()))


# ---- selection ---------------------------------------------------------------------------------------------------------------------------
def _crafted_masks():
    """class 3 everywhere; sample 0 and 1: a two-class patch (5 | 7) in the top-left 20 x 40 source pixels; sample 1 also (1 | 2) in the
    bottom-right 10 x 18; sample 2: all void but one corner of class 4"""
    m = np.full((N, HS, WS), 3, dtype=np.uint8)
    m[:2, :20, :20] = 5
    m[:2, :20, 20:40] = 7
    m[1, 35:, 65:74] = 1
    m[1, 35:, 74:] = 2
    m[2] = VOID
    m[2, :5, :5] = 4
    return m


# at ratio 2 (90 x 166, steps 1/2) the 33 x 70 window at (0, 0) shows 40 columns of 5 and 30 of 7: passes; at (0, 70) 10 columns of 7
# and 60 of 3: two classes at 6/7 > 0.75, fails; at (40, 50) class 3 alone: fails
PASS, HEAVY, ONE = (0, 0), (0, 70), (40, 50)


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_selection_and_counts_equal_the_restatement(mask_dtype):
    frames, _ = C.frames_masks()
    masks = _crafted_masks()
    up = dict(Hr=90, Wr=166, sy=0.5, sx=0.5)
    first = [_p(**up, cands=[PASS] + [ONE] * 10),                                     # candidate 0 passes
             _p(**up, cands=[ONE, HEAVY, ONE, HEAVY, ONE, HEAVY, ONE, PASS, HEAVY, ONE, ONE], flip=True),   # only candidate 7 passes
             _p(**up, cands=[ONE] * 11)]                                               # sample 2 is void there: nothing counted
    second = [_p(**up, cands=[HEAVY, ONE] * 5 + [PASS]),                               # none passes; the fallback would, untested
              _p(**up, cands=[(70, 130)] + [ONE] * 10),                                # 20 x 36 of the window inside: (1 | 2), pad not counted
              _p(23, 42, HS / 23, WS / 42, cands=[(-5, -14)] * 11)]                    # centred pad; class 4 + void is one class
    want_sel = [[(0, 0, 0, 1), (7, 0, 0, 1), (10, 40, 50, 0)], [(10, 0, 0, 0), (0, 70, 130, 1), (10, -5, -14, 0)]]
    for params, expect in zip((first, second), want_sel):
        x, m, u8, counts, sel, rec = _run(frames, masks, params, mask_dtype=mask_dtype)
        rc, rs = C.selection_tables(masks, rec, HC, WC, VOID, 0.75)
        assert np.array_equal(counts, rc) and np.array_equal(sel, rs)
        assert [tuple(r) for r in sel.tolist()] == expect
        mh = m.cpu().numpy()
        for n in range(N):                                                             # the chosen window is the one that was cut
            shown = mh[n][mh[n] != VOID]
            assert np.array_equal(np.bincount(shown, minlength=256).astype(np.uint32), counts[n, sel[n, 0]]), n
            assert np.array_equal(mh[n], _ref(frames, masks, rec, sel)[n][1]), n
    assert counts[1, 0].sum() == 20 * 36 and counts[1, 0, 1] == counts[1, 0, 2] == 360
    assert counts[2].sum() == 11 * 3 * 3 and counts[0, 0].sum() == 33 * 70             # 5 x 5 of class 4 at half size: rows 0..2
    # cat_max_ratio = 1 with one candidate tests nothing; the later candidates' rows stay cleared
    x, m, u8, counts, sel, rec = _run(frames, masks, [_p(**up, cands=[c]) for c in (ONE, HEAVY, PASS)], ratio=1.0, mask_dtype=mask_dtype)
    assert sel.tolist() == [[0, 40, 50, 0], [0, 0, 70, 0], [0, 0, 0, 0]]
    rc, rs = C.selection_tables(masks, rec, HC, WC, VOID, 1.0)
    assert np.array_equal(counts, rc) and np.array_equal(sel, rs) and not counts[:, 1:].any()


def test_exact_equality_of_max_over_sum_and_the_ratio_fails():
    """3/4 of the counted pixels in one class: max / sum == 0.75 exactly, not < 0.75; one pixel fewer passes"""
    frames, _ = C.frames_masks()
    masks = np.full((N, HS, WS), 3, dtype=np.uint8)
    masks[:, :8, :10] = 5                                                              # window 32 x 10 at (0, 0): 8 rows of 5, 24 of 3
    masks[1, 8, 0] = 5                                                                 # sample 1: 239 / 320 < 0.75
    masks[2, 0, 0] = VOID                                                              # sample 2: 240 / 319 > 0.75
    params = [_p(HS, WS, 1.0, 1.0, cands=[(0, 0), (1, 1)])] * 3
    x, m, u8, counts, sel, rec = _run(frames, masks, params, hc=32, wc=10)
    assert counts[:, 0, 3].tolist() == [240, 239, 240] and counts[:, 0, 5].tolist() == [80, 81, 79]
    assert sel[:, [0, 3]].tolist() == [[1, 0], [0, 1], [1, 0]]
    assert np.array_equal(sel, C.selection_tables(masks, rec, 32, 10, VOID, 0.75)[1])


# ---- masks and geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_normalized", [0, 1])
@pytest.mark.parametrize("flip", [False, True])
def test_masks_pad_and_normalisation_are_exact(flip, pad_normalized):
    frames, masks = C.frames_masks(seed=1)
    params = [_p(62, 114, HS / 62, WS / 114, [(20, 30)], flip),                        # larger than the crop
              _p(27, 51, HS / 27, WS / 51, [(0, 0)], flip, jitter=[("contrast", 1.3)]),   # smaller in both: pad bottom and right
              _p(27, 51, 1 / 0.61, 1 / 0.61, [(-3, -9)], flip)]                        # centred pad: negative offsets
    x, m, u8, counts, sel, rec = _run(frames, masks, params, ratio=1.0, pad_normalized=pad_normalized)
    ref = _ref(frames, masks, rec, sel)
    mh, uh = m.cpu().numpy(), u8.cpu().numpy()
    black = A.preprocess_uint8(torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=DEV))[0, :, 0, 0]
    full = A.preprocess_uint8(u8)
    assert x._base is not None and x._base.shape == (N, HC, WC, 4) and not x._base[..., 3].any()
    for n in range(N):
        want_u8, want_m, inside = ref[n]
        assert np.array_equal(mh[n], want_m), n
        assert (mh[n][~inside] == VOID).all() and (uh[n][~inside] == 0).all()
        assert inside.sum() == [HC * WC, 27 * 51, 27 * 51][n]
        ins = torch.from_numpy(inside).to(DEV)
        xn = x[n].permute(1, 2, 0)
        assert torch.equal(xn[ins], full[n].permute(1, 2, 0)[ins])                    # bitwise preprocess_uint8 of the uint8 output
        if n:
            pad = xn[~ins]
            assert torch.equal(pad, black.expand_as(pad)) if pad_normalized else not pad.any()
    # int64 labels pass through untruncated, pad included
    big = masks.astype(np.int64) * 1000
    x2, m2, u2, _, sel2, _ = _run(frames, big, params, ratio=1.0, pad_label=VOID * 1000, pad_normalized=pad_normalized, mask_dtype=torch.int64)
    assert torch.equal(m2, m * 1000) and torch.equal(x2, x) and torch.equal(u2, u8) and np.array_equal(sel2, sel)


# ---- image values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0.5, 1.0, 2.0])
def test_dyadic_steps_are_bitwise(step):
    Hs, Ws = 46, 84
    frames, masks = C.frames_masks(N, Hs, Ws, seed=2)
    Hr, Wr = int(Hs / step), int(Ws / step)                                            # 92 x 168, 46 x 84, 23 x 42
    offs = {0.5: [(0, 0), (59, 98), (40, 120)], 1.0: [(0, 0), (13, 14), (-7, 30)], 2.0: [(0, 0), (-5, -14), (-10, -28)]}[step]
    params = [_p(Hr, Wr, step, step, [offs[0]]), _p(Hr, Wr, step, step, [offs[1]], flip=True, jitter=[("brightness", 1.2)]),
              _p(Hr, Wr, step, step, [offs[2]], flip=True)]
    x, m, u8, counts, sel, rec = _run(frames, masks, params, ratio=1.0)
    for n, (want_u8, want_m, inside) in enumerate(_ref(frames, masks, rec, sel)):
        assert np.array_equal(u8[n].cpu().numpy(), want_u8), (n, int((u8[n].cpu().numpy() != want_u8).sum()))
        assert np.array_equal(m[n].cpu().numpy(), want_m), n


def test_step_one_zero_offset_full_crop_is_preprocess_uint8():
    frames, masks = C.frames_masks(seed=3)
    x, m, u8, counts, sel, rec = _run(frames, masks, [_p(HS, WS, 1.0, 1.0, [(0, 0)])] * N, hc=HS, wc=WS, ratio=1.0)
    gf = torch.from_numpy(frames).to(DEV)
    assert torch.equal(u8, gf) and torch.equal(x, A.preprocess_uint8(gf)) and torch.equal(m.cpu(), torch.from_numpy(masks).long())


@pytest.mark.parametrize("case", C.step_cases(), ids=[c[0] for c in C.step_cases()])
def test_other_ratios_differ_only_inside_the_rounding_band(case):
    name, Hr, Wr, sy, sx = case
    frames, masks = C.frames_masks()                                                   # the inputs the CPU test bounds the band's share for
    offs = [(0, 0), (max(Hr - HC, 0), max(Wr - WC, 0)), (-4, Wr - WC + 9)]            # flush corners; pad on top and on the right
    params = [_p(Hr, Wr, sy, sx, [offs[0]]), _p(Hr, Wr, sy, sx, [offs[1]], jitter=[("brightness", 1.3), ("contrast", 0.8)]),
              _p(Hr, Wr, sy, sx, [offs[2]], flip=True)]
    x, m, u8, counts, sel, rec = _run(frames, masks, params, ratio=1.0)
    uh = u8.cpu().numpy()
    for n, (want_u8, want_m, inside) in enumerate(_ref(frames, masks, rec, sel)):
        near = C.near_half(C.resize_linear_pre(frames[n], Hr, Wr, sy, sx), C.DELTA_RESIZE)
        _check_values(uh[n], want_u8, _band(near, rec[n], sel[n]), rec[n], (name, n))
        assert np.array_equal(m[n].cpu().numpy(), want_m), (name, n)


@pytest.mark.parametrize("blur", C.BLURS, ids=["k3", "k9"])
def test_blur_of_the_kernels_own_resized_values(blur):
    """the blur restated in fp64 on the kernel's own unblurred resized image (a run whose crop is the whole resized image), so that
    first-stage rounding differences do not propagate"""
    k, sigma = blur
    frames, masks = C.frames_masks()
    Hr, Wr = 62, 114
    sy, sx = HS / Hr, WS / Wr
    whole = _run(frames, masks, [_p(Hr, Wr, sy, sx, [(0, 0)])] * N, hc=Hr, wc=Wr, ratio=1.0)[2].cpu().numpy()
    # top-left corner: the halo reflects at two borders; flush bottom-right; overhanging: pad rows above, pad columns next to the image
    offs = [(0, 0), (Hr - HC, Wr - WC), (-5, 60)]
    params = [_p(Hr, Wr, sy, sx, [offs[0]], blur=blur), _p(Hr, Wr, sy, sx, [offs[1]], flip=True, blur=blur),
              _p(Hr, Wr, sy, sx, [offs[2]], blur=blur, jitter=[("contrast", 1.2)])]
    x, m, u8, counts, sel, rec = _run(frames, masks, params, ratio=1.0)
    uh = u8.cpu().numpy()
    for n in range(N):
        pre = C.blur_pre(whole[n], rec[n]["taps"][:k].astype(np.float64))
        want = C.round_u8(pre)
        if rec[n]["use_lut"]:
            want = rec[n]["lut"][want]
        want, inside = C.window(want, HC, WC, *offs[n], 0)
        if rec[n]["flip"]:
            want, inside = want[:, ::-1], inside[:, ::-1]
        _check_values(uh[n], want, _band(C.near_half(pre, C.blur_delta(k)), rec[n], sel[n]), rec[n], (k, n))
        assert (uh[n][~inside] == 0).all() and inside.sum() == [HC * WC, HC * WC, 28 * 54][n]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_seeded_crop_transforms_equal_the_restatement_under_the_same_draws():
    frames, masks = C.frames_masks()
    tf = T.crop_transforms(crop_size=(HC, WC))
    random.seed(4)
    x, m, u8 = tf(torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), out_u8=True)
    sel = tf.last_selection.cpu().numpy()
    random.seed(4)
    rec = T.CropCompose.pack([tf.draw(HS, WS) for _ in range(N)])
    assert np.array_equal(sel, C.selection_tables(masks, rec, HC, WC, VOID, 0.75)[1])
    assert (rec["ncand"] == 11).all()
    uh = u8.cpu().numpy()
    for n, (want_u8, want_m, inside) in enumerate(_ref(frames, masks, rec, sel)):
        r = rec[n]
        near = C.near_half(C.resize_linear_pre(frames[n], int(r["Hr"]), int(r["Wr"]), float(r["sy"]), float(r["sx"])), C.DELTA_RESIZE)
        assert near.mean() <= 0.01
        _check_values(uh[n], want_u8, _band(near, r, sel[n]), r, n)
        assert np.array_equal(m[n].cpu().numpy(), want_m), n
        ins = torch.from_numpy(inside).to(DEV)
        xn = x[n].permute(1, 2, 0)
        assert not xn[~ins].any() and torch.equal(xn[ins], A.preprocess_uint8(u8)[n].permute(1, 2, 0)[ins])
    # the same seeded batch twice: bitwise equal
    random.seed(4)
    x2, m2, u2 = tf(torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), out_u8=True)
    assert torch.equal(x2, x) and torch.equal(m2, m) and torch.equal(u2, u8) and np.array_equal(tf.last_selection.cpu().numpy(), sel)


@pytest.mark.parametrize("mask_dtype", [np.uint8, np.int64])
def test_device_prefetcher_with_crop_transforms_matches_direct_calls(mask_dtype):
    batches = [C.frames_masks(2, HS, WS, 100 + b) for b in range(3)]
    batches = [(f, mk.astype(mask_dtype)) for f, mk in batches]
    tf = T.crop_transforms(crop_size=(HC, WC), blur=True)
    random.seed(3)
    got = [(x.clone(), m.clone()) for x, m in A.DevicePrefetcher(batches, transforms=tf)]
    random.seed(3)
    want = [tf(torch.from_numpy(f).to(DEV), torch.from_numpy(mk).to(DEV)) for f, mk in batches]
    assert len(got) == len(want) == 3
    for (gx, gm), (wx, wm) in zip(got, want):
        assert gx.shape == (2, 3, HC, WC) and gm.dtype == torch.int64 and gm.shape == (2, HC, WC)
        assert torch.equal(gx, wx) and torch.equal(gm, wm)
    sj = T.CropCompose([T.ScaleJitter(), T.RandomHorizontalFlip(), T.ToTensor(), T.Normalize(T.CAMVID_MEAN, T.CAMVID_STD)])
    random.seed(5)
    got = [(x.clone(), m.clone()) for x, m in A.DevicePrefetcher(batches, transforms=sj)]
    random.seed(5)
    for (gx, gm), (f, mk) in zip(got, batches):
        wx, wm = sj(torch.from_numpy(f).to(DEV), torch.from_numpy(mk).to(DEV))
        assert gx.shape == (2, 3, HS, WS) and torch.equal(gx, wx) and torch.equal(gm, wm)


def test_fixed_pipeline_through_the_prefetcher_is_unchanged():
    from tests import augment_ref as R
    batches = [C.frames_masks(2, HS, WS, 200 + b) for b in range(2)]
    tr = T.train_transforms(image_size=(WC, HC))
    random.seed(6)
    got = [(x.clone(), m.clone()) for x, m in A.DevicePrefetcher(batches, transforms=tr)]
    random.seed(6)
    for (gx, gm), (f, mk) in zip(got, batches):
        params = [tr.draw() for _ in range(2)]
        rec = T.Compose.pack(params)
        wx, wm = T.augment_u8(torch.from_numpy(f).to(DEV), torch.from_numpy(mk).to(DEV), torch.from_numpy(rec.view(np.uint8)).to(DEV), (HC, WC))
        assert torch.equal(gx, wx) and torch.equal(gm, wm)
        for n in range(2):
            assert np.array_equal(gm[n].cpu().numpy(), R.augment(f[n], mk[n], HC, WC, flip=params[n]["flip"])[1])


def test_few_training_steps_on_crops():
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(DEV).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    loss_fn = A.CrossEntropyLoss()
    g = torch.Generator().manual_seed(5)
    blobs = torch.nn.functional.interpolate((torch.rand(4, 1, 12, 16, generator=g) * 12).floor(), size=(192, 256), mode="nearest")
    masks = blobs[:, 0].to(torch.uint8)
    frames = ((masks.long().unsqueeze(-1) * torch.tensor([20, 15, 10])) % 256).to(torch.uint8).numpy()
    tf = T.crop_transforms(crop_size=(96, 128))
    random.seed(0)
    losses = []
    for x, m in A.DevicePrefetcher([(frames, masks.numpy())] * 12, transforms=tf):
        assert x.shape == (4, 3, 96, 128) and m.shape == (4, 96, 128)
        opt.zero_grad()
        loss = loss_fn(net(x), m)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-3:]) < losses[0], losses
