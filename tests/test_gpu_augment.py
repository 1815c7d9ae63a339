"""The device transforms (cvk_augment_u8 via pytorch_camvid_amd.transforms) against the fp64 restatement in tests/augment_ref.py.
Exactness: flip, nearest mask resize, LUT and normalisation are bitwise; the 2:1 bilinear downscale (weights of exactly 1/2) is
exact; other ratios and the blur allow 1 level on <= 0.1 % of the uint8 values (fp32 taps and sums near .5 boundaries)."""
import os
import random

import numpy as np
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import transforms as T

from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (ksize, sigma) near both ends of each bucket of RandomGaussianBlur's ksize rule, and no blur
BLURS = [(0, 0.0), (3, 0.05), (3, 1.2), (5, 1.22), (5, 1.8), (7, 1.83), (7, 2.42), (9, 2.43), (9, 2.99)]
SHAPES = [(2, 720, 960, 360, 480), (3, 250, 333, 96, 128), (2, 100, 150, 181, 241)]


def _frames(N, Hs, Ws, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8), g.integers(0, 12, (N, Hs, Ws), dtype=np.uint8)


def _params(N, k, sigma, seed):
    g = random.Random(seed)
    out = []
    for i in range(N):
        jitter = [] if i % 2 == 0 else [("brightness", g.uniform(0.6, 1.4)), ("contrast", g.uniform(0.6, 1.4))]
        out.append({"flip": bool(i % 2 == (seed & 1)), "blur": (k, sigma) if k else None, "jitter": jitter or None})
    return out


def _run(frames, masks, params, H, W, mask_dtype=torch.uint8):
    rec = T.Compose.pack(params)
    grec = torch.from_numpy(rec.view(np.uint8)).to(DEV)
    x, m, u8 = T.augment_u8(torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV).to(mask_dtype), grec, (H, W),
                            out_u8=True)
    torch.cuda.synchronize()
    return x, m, u8, rec


def _check(frames, masks, params, rec, x, m, u8, H, W, exact):
    u8h, mh = u8.cpu().numpy(), m.cpu().numpy()
    for i, p in enumerate(params):
        k = p["blur"][0] if p["blur"] else 0
        ref, refm = R.augment(frames[i], masks[i], H, W, k, rec[i]["taps"].astype(np.float64), p["flip"],
                              rec[i]["lut"] if rec[i]["use_lut"] else None)
        assert np.array_equal(mh[i], refm.astype(np.int64)), i
        d = np.abs(u8h[i].astype(np.int32) - ref.astype(np.int32))
        if exact:
            assert d.max() == 0, (i, int(d.max()), int((d > 0).sum()))
        else:
            # LUT stages can turn a 1-level difference into a larger one: compare before the table where it was applied
            assert (d > 0).mean() <= 1e-3, (i, p, int((d > 0).sum()))
            if rec[i]["use_lut"]:
                lut = rec[i]["lut"].astype(np.int32)
                steps = np.abs(np.diff(lut)).max()
                assert d.max() <= max(1, steps), (i, int(d.max()))
            else:
                assert d.max() <= 1, (i, int(d.max()))
    # normalisation: bitwise the float output preprocess_uint8 makes of the uint8 frames
    assert torch.equal(x, A.preprocess_uint8(u8))


@pytest.mark.parametrize("shape", SHAPES, ids=["720x960to360x480", "250x333to96x128", "upscale100x150to181x241"])
def test_forced_parameters_against_restatement(shape):
    N, Hs, Ws, H, W = shape
    frames, masks = _frames(N, Hs, Ws, Hs)
    for j, (k, sigma) in enumerate(BLURS):
        params = _params(N, k, sigma, j)
        x, m, u8, rec = _run(frames, masks, params, H, W)
        assert x.shape == (N, 3, H, W) and x.dtype == torch.float32 and m.dtype == torch.int64
        _check(frames, masks, params, rec, x, m, u8, H, W, exact=(k == 0 and Hs == 2 * H and Ws == 2 * W))


def test_int64_masks_and_no_u8_output():
    N, Hs, Ws, H, W = 2, 250, 333, 96, 128
    frames, masks = _frames(N, Hs, Ws, 7)
    params = _params(N, 5, 1.5, 3)
    x8, m8, u8, rec = _run(frames, masks, params, H, W)
    x64, m64, _, _ = _run(frames, masks, params, H, W, mask_dtype=torch.int64)
    big = torch.from_numpy(masks.astype(np.int64) * 1000).to(DEV)      # int64 labels pass through untruncated
    x2, mbig = T.augment_u8(torch.from_numpy(frames).to(DEV), big, torch.from_numpy(rec.view(np.uint8)).to(DEV), (H, W))
    assert torch.equal(x8, x64) and torch.equal(m8, m64) and torch.equal(x2, x8) and torch.equal(mbig, m8 * 1000)


def test_nothing_fired_equals_preprocess_uint8():
    frames, masks = _frames(3, 360, 480, 11)
    f = torch.from_numpy(frames).to(DEV)
    x, m = T.valid_transforms()(f, torch.from_numpy(masks).to(DEV))
    assert torch.equal(x, A.preprocess_uint8(f))
    assert torch.equal(m.cpu(), torch.from_numpy(masks).long())


def test_seeded_train_transforms_match_the_reference_draws(golden_dir):
    fx = np.load(os.path.join(golden_dir, "aug_params.npz"))
    N, Hs, Ws, H, W = 8, 720, 960, 360, 480
    frames, masks = _frames(N, Hs, Ws, 21)
    random.seed(0)
    x, m, u8 = T.train_transforms()(torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), out_u8=True)
    torch.cuda.synchronize()
    params = []
    for i in range(N):
        k, s = int(fx["train_s0_ksize"][i]), float(fx["train_s0_sigma"][i])
        params.append({"flip": bool(fx["train_s0_flipped"][i]), "blur": (k, s) if k else None, "jitter": None})
    rec = T.Compose.pack(params)
    rec["lut"] = fx["train_s0_lut"][:N]
    rec["use_lut"] = fx["train_s0_jittered"][:N]
    _check(frames, masks, params, rec, x, m, u8, H, W, exact=False)


@pytest.mark.parametrize("mask_dtype", [np.uint8, np.int64])
def test_device_prefetcher_with_transforms_matches_direct_calls(mask_dtype):
    N, Hs, Ws = 2, 720, 960
    batches = [_frames(N, Hs, Ws, 100 + b) for b in range(3)]
    batches = [(f, mk.astype(mask_dtype)) for f, mk in batches]
    tr = T.train_transforms()
    random.seed(3)
    got = [(x.clone(), m.clone()) for x, m in A.DevicePrefetcher(batches, transforms=tr)]
    random.seed(3)
    want = [tr(torch.from_numpy(f).to(DEV), torch.from_numpy(mk).to(DEV)) for f, mk in batches]
    assert len(got) == len(want) == 3
    for (gx, gm), (wx, wm) in zip(got, want):
        assert gx.shape == (N, 3, 360, 480) and gm.dtype == torch.int64
        assert torch.equal(gx, wx) and torch.equal(gm, wm)


def test_few_training_steps_fed_by_the_device_transforms():
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(DEV).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    loss_fn = A.CrossEntropyLoss()
    g = torch.Generator().manual_seed(5)
    blobs = torch.nn.functional.interpolate((torch.rand(4, 1, 12, 16, generator=g) * 12).floor(), size=(192, 256), mode="nearest")
    masks = blobs[:, 0].to(torch.uint8)
    frames = ((masks.long().unsqueeze(-1) * torch.tensor([20, 15, 10])) % 256).to(torch.uint8).numpy()
    tr = T.train_transforms(image_size=(128, 96))
    random.seed(0)
    losses = []
    for x, m in A.DevicePrefetcher([(frames, masks.numpy())] * 12, transforms=tr):
        opt.zero_grad()
        loss = loss_fn(net(x), m)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-3:]) < losses[0], losses
