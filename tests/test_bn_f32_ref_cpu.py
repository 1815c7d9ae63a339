"""tests/bn_f32_ref.py is right, and the inputs of tests/test_gpu_bn_f32.py are what its tests assume: checked here without a GPU.
The restatements of the statistics, with UNROUNDED fp64 partials, are held against torch's batch_norm in fp64 (1e-12 relative to the
tensors' scale: two orders of evaluation); the E planes against the interpolation points of F(4,3) and against a literal
transcription of the four formulas; the padded layout against its description.  The GPU file's generators run here too: no backward case
may hold an element whose ReLU mask is ambiguous in fp32, every case holds the exact-zero edge, the statistics cases reach every branch
of the level-1 kernel's group and loop arithmetic, and the rounding bound of the partials dominates its first-order derivation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_f32_ref as S
from tests import elem_bf16_ref as R
from tests import test_gpu_bn_f32 as G

EPS = 1e-5
TIGHT = 1e-12


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) <= TIGHT * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("M,C,ragged", [(71, 5, False), (64, 3, False), (200, 7, False), (200, 7, True), (2, 4, False)])
def test_finalisation_of_unrounded_partials_matches_torch_batch_norm(M, C, ragged):
    g = torch.Generator().manual_seed(M + C)
    y = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.3 + 0.7
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    counts = [1, 130, 3, 66] if ragged else S.granule_counts(M)
    stats = S.partials(y.numpy(), counts, dtype=np.float64)
    eps, mom = float(np.float32(EPS)), float(np.float32(0.1))
    r = S.finalize(stats, counts, M, gamma.numpy(), beta.numpy(), EPS, 0.1, rm.numpy(), rv.numpy())
    trm, trv = rm.clone(), rv.clone()
    want = F.batch_norm(y, trm, trv, gamma, beta, training=True, momentum=mom, eps=eps)
    assert close(r["mean"], y.mean(0)) and close(r["var"], y.var(0, unbiased=False)) and close(r["unbiased"], y.var(0, unbiased=True))
    assert close(r["running_mean"], trm) and close(r["running_var"], trv)
    assert close(R.apply(y, torch.from_numpy(r["scale"].astype(np.float64)), torch.from_numpy(r["shift"].astype(np.float64))), F.relu(want))
    assert close(r["rstd"], (y.var(0, unbiased=False) + eps).rsqrt())
    # the magnitudes the bounds are written in
    s = stats[0]
    n = np.asarray(counts, dtype=np.float64)[:, None]
    assert close(r["abs_s"], np.abs(s).sum(0)) and close(r["round_mag"], stats[1].sum(0) + 2 * (s * s / n).sum(0))
    assert close(r["var_mag"], stats[1].sum(0) + (s * s / n).sum(0) + s.sum(0) ** 2 / M)


def test_one_row_uses_the_biased_variance_for_the_running_estimate():
    y = np.array([[1.5, -2.0]])
    r = S.finalize(S.partials(y, [1]), [1], 1, np.ones(2), np.zeros(2), EPS, 0.1, np.zeros(2), np.ones(2))
    assert r["var"].tolist() == [0, 0] and r["unbiased"].tolist() == [0, 0]
    assert close(r["running_var"], [1 - float(np.float32(0.1))] * 2) and close(r["rstd"], [1 / np.sqrt(float(np.float32(EPS)))] * 2)


def test_partials_layout_and_granules():
    assert S.granule_counts(1) == [1] and S.granule_counts(64) == [64] and S.granule_counts(71) == [64, 7] and len(S.granule_counts(6353)) == 100
    y = np.arange(12, dtype=np.float64).reshape(6, 2)
    p = S.partials(y, [4, 2])
    assert p.dtype == np.float32 and p.shape == (2, 2, 2)
    assert p[0].tolist() == [[12.0, 16.0], [18.0, 20.0]] and p[1].tolist() == [[20.0, 20.0], [2.0, 2.0]]


def test_negative_m2_is_clamped():
    """a combination that comes out negative (forced here by a negative q, which no real partial has) is variance 0, not NaN"""
    r = S.finalize(np.array([[[3.0], [1.0]], [[-1e-3], [0.0]]], dtype=np.float32), [3, 1], 4, [1.0], [0.0], EPS)
    assert float(r["var"][0]) == 0.0 and float(r["unbiased"][0]) == 0.0 and close(r["rstd"], [1 / np.sqrt(float(np.float32(EPS)))])


def test_eval_params_match_torch_eval_mode():
    g = torch.Generator().manual_seed(5)
    C = 9
    y = torch.randn(30, C, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    r = S.eval_params(gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy(), EPS)
    want = F.relu(F.batch_norm(y, rm, rv, gamma, beta, training=False, eps=float(np.float32(EPS))))
    assert close(R.apply(y, torch.from_numpy(r["scale"].astype(np.float64)), torch.from_numpy(r["shift"].astype(np.float64))), want)
    assert close(r["mean"], rm) and close(r["rstd"], (rv + float(np.float32(EPS))).rsqrt())


@pytest.mark.parametrize("W", [4, 7, 12, 13])
def test_e_planes(W):
    """E1..E4 evaluate the cubic d0 + d1 p + d2 p^2 + d3 p^3 at p = 1, -1, 2, -2; E0 and E5 are its lowest and highest coefficient; the
    literal formulas of the kernel's header comment; columns past W are zero."""
    g = torch.Generator().manual_seed(W)
    N, H, C = 2, 3, 5
    dy = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    E = S.e_planes(dy)
    Wt = -(-W // 4)
    assert E.shape == (6, N, H, Wt, C)
    pad = torch.zeros(N, H, 4 * Wt, C, dtype=torch.float64)
    pad[:, :, :W] = dy
    d0, d1, d2, d3 = (pad[:, :, i::4] for i in range(4))
    want = [d0, d0 + d1 + d2 + d3, d0 - d1 + d2 - d3, d0 + 2 * d1 + 4 * d2 + 8 * d3, d0 - 2 * d1 + 4 * d2 - 8 * d3, d3]
    for k in range(6):
        assert close(E[k], want[k])
    for k, p in enumerate(S.E_POINTS):
        assert close(E[1 + k], d0 + p * (d1 + p * (d2 + p * d3)))
    assert close(S.e_planes(dy.abs(), S.E_COEF.abs())[4], d0.abs() + 2 * d1.abs() + 4 * d2.abs() + 8 * d3.abs())


@pytest.mark.parametrize("shape", [(2, 9, 12), (2, 9, 13), (1, 1, 1), (3, 2, 33)])
def test_padded_layout(shape):
    """Every (n, y, xt) has a row of its own inside the plane; what is left are the pad rows: Wtp first, Wtp last, one row of Wtp above... in
    all 2 Wtp + 2 N Wtp + N H (Wtp - Wt), the count csrc/wgradp.hip's zeroing pass covers."""
    N, H, W = shape
    Wt = -(-W // 4)
    Wtp, rows, prow = S.padded_layout(N, H, W)
    assert Wtp % 8 == 0 and 0 <= Wtp - Wt < 8 and rows == N * (H + 2) * Wtp + 2 * Wtp
    flat = prow.reshape(-1)
    assert prow.shape == (N, H, Wt) and len(set(flat.tolist())) == flat.numel() and int(flat.min()) >= 2 * Wtp and int(flat.max()) < rows - 2 * Wtp + Wt
    assert rows - flat.numel() == 2 * Wtp + 2 * N * Wtp + N * H * (Wtp - Wt)
    assert int(prow[0, 0, 0]) == 2 * Wtp and (N == 1 or int(prow[1, 0, 0]) - int(prow[0, H - 1, 0]) == 3 * Wtp)      # two pad rows between images


# ------------------------------------------------------------------------------------------------ the GPU file's inputs
BACKWARD = {**{k: v[0] for k, v in G.BN_CASES.items()}, **{k: v[0] for k, v in G.E_CASES.items()}, **G.E6_CASES}
FORWARD = {**{k: v[0] for k, v in G.APPLY_CASES.items()}, **{k: v[0] for k, v in G.POOL_CASES.items()}}


@pytest.mark.parametrize("name", list(BACKWARD))
def test_backward_cases_hold_no_ambiguous_element_and_the_zero_edge(name):
    """Zero elements in the exclusion band (the cap is 0 at these sizes, 1 for the one of 156 000 elements), and in channel 0 elements
    with z == 0 exactly, whose mask is False."""
    shape = BACKWARD[name]
    inp = G.bn_inputs(shape, G.case_seed(name))
    assert all(v.dtype == torch.float32 for v in inp.values())
    q = {k: v.double() for k, v in inp.items()}
    mask, g, gx, band = R.bn_bwd_terms(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"])
    assert int(band.sum()) == 0 and G.excluded_cap(band.numel()) <= 1
    assert band.numel() <= 156000
    z0 = (q["y"][:, 0] * q["scale"][0] + q["shift"][0]) == 0
    assert int(z0.sum()) >= q["y"].shape[0] // 3 and not bool(mask[:, 0][z0].any())
    assert bool(mask.any()) and not bool(mask.all())


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_cases_hold_the_zero_edge_and_both_signs(name):
    inp = G.bn_inputs(FORWARD[name], G.case_seed(name))
    z = inp["y"].double() * inp["scale"].double() + inp["shift"].double()
    assert bool((z[:, 0] == 0).any()) and bool((z > 0).any()) and bool((z < 0).any())


def test_case_tables_name_the_vector_width_their_layout_selects():
    for name, (shape, ldy, kind, V) in G.BN_CASES.items():
        lay = G.Lay(shape, **G.DOUT_LAYOUTS[kind])
        assert V == G.expect_v4(shape[3], [ldy], lay) == G.expect_v4(shape[3], [ldy, shape[3] + 4], lay), name
        assert name.startswith(f"v{V}_")
    for name, (shape, ldy, lay_kw, V, off) in G.APPLY_CASES.items():
        assert V == G.expect_v4(shape[3], [ldy], G.Lay(shape, **lay_kw), [off]) and name.startswith(f"v{V}_"), name
    for name, (shape, ldy, lay_kw) in G.POOL_CASES.items():
        assert G.expect_v4(shape[3], [ldy], G.Lay(shape, **lay_kw)) == 4, name
    assert {V for _, _, _, V in G.BN_CASES.values()} == {1, 4}


def level1_walk(P):
    """(G, rows per group, whether any lane runs the two-chain loop, whether any runs its tail, whether a group is ragged) by the
    arithmetic of cvk_bn_finalize and k_bn_stats_l1"""
    Gn = 1 if P < 32 else min(P // 32, 64)
    rpg = -(-P // Gn)
    two = tail = False
    covered = []
    for grp in range(Gn):
        pbeg, pend = grp * rpg, min(P, (grp + 1) * rpg)
        for lane in range(4):
            p = pbeg + lane
            while p + 4 < pend:
                covered += [p, p + 4]
                two = True
                p += 8
            while p < pend:
                covered.append(p)
                tail = True
                p += 4
    assert sorted(covered) == list(range(P))
    return Gn, rpg, two, tail, P % rpg != 0


def test_statistics_cases_reach_every_branch_of_the_level_one_kernel():
    P = {name: len(S.granule_counts(M)) for name, M in G.STAT_M.items()}
    assert [P[k] for k in ("m1", "m64", "m71", "p5", "p8", "p9", "p31", "p33", "p100")] == [1, 1, 2, 5, 8, 9, 31, 33, 100]
    assert G.STAT_M["m71"] % 64 == 7 and G.STAT_M["p8"] % 64 == 0
    assert level1_walk(1)[:4] == (1, 1, False, True) and level1_walk(2)[2] is False
    assert level1_walk(5)[2] and level1_walk(8)[2:4] == (True, False) and level1_walk(9)[2:4] == (True, True)
    assert level1_walk(31)[0] == 1 and level1_walk(33)[:2] == (1, 33)
    assert level1_walk(100) == (3, 34, True, True, True) and level1_walk(2100) == (64, 33, True, True, True)
    assert set(G.STAT_C) == {1, 63, 64, 65, 130}


@pytest.mark.parametrize("name,ragged", [(n, r) for n in G.STAT_CASES for r in (False, True)] + [(n, False) for n in G.STAT_SPECIAL])
def test_statistics_problems_are_what_the_gpu_tests_assume(name, ragged):
    """Counts sum to M, q_p >= 0, P is ceil(M/64) for the granule form; for the cases drawn from a tensor the stated rounding bound of
    the partials, u (sum q_p + 2 sum s_p^2/n_p), dominates the first-order effect 2u sum|s_p| |s_p/n_p - S/M| + u sum q_p of rounding them."""
    for C in ((5,) if name in G.STAT_SPECIAL else G.STAT_C):
        prob = G.stat_problem(name, C, ragged)
        stats, counts, M = prob["stats"], prob["counts"], prob["M"]
        assert stats.dtype == np.float32 and stats.shape == (2, len(counts), C) and sum(counts) == M and bool((stats[1] >= 0).all())
        if not ragged:
            assert counts == S.granule_counts(M) and len(counts) == -(-M // 64)
        if prob["y"] is None:
            assert len(counts) == 2100
            continue
        assert prob["y"].shape == (M, C) and np.array_equal(prob["y"], prob["y"].astype(np.float32).astype(np.float64))
        s = stats[0].astype(S.LD)
        n = np.asarray(counts, dtype=S.LD)[:, None]
        first_order = 2 * (np.abs(s) * np.abs(s / n - s.sum(0) / M)).sum(0)
        assert bool((first_order <= 2 * (s * s / n).sum(0)).all()), name
    if name == "illcond_m4544":
        assert M == 71 * 64 and abs(float(prob["y"].mean()) - 100) < 0.01 and abs(float(prob["y"].std()) - 0.01) < 0.001
    if name == "constant_m71":
        assert bool((prob["y"] == prob["y"][0]).all()) and bool((stats[1] == 0).all()) and prob["y"][0, 0] == 0 and len(set(prob["y"][0].tolist())) == C
