"""CPU (no GPU): the case tables, references and bounds of tests/analysis_ref.py, which tests/test_analysis_parity_gpu.py
applies to the evaluation / analysis kernels.

  * every case reaches the branch it is named for, computed from the constants `analysis_ref.geometry()` reads out of the
    launchers' source lines: a grid cap, a per-workgroup count or the top-k instance chain edited without re-sizing the
    case fails here and names the case;
  * the reference-only conditions the GPU checks rely on hold (|lse| > 1, enough probabilities above the floor, the
    exact-value cases exact in float64);
  * the comparisons can fail: references carrying one mistake each differ from the true one by more than the tolerance
    on the case meant for that mistake.
"""
import math

import pytest
import torch

from tests import analysis_ref as ar
from tests import parity_util as pu

G = ar.geometry()
DTYPES = [torch.float32, torch.float16]


# ---- geometry -------------------------------------------------------------------------------------------------------
def test_the_launchers_constants_are_the_ones_the_cases_were_sized_for():
    """A change here is no error of the launcher's: it means the cases below must be re-sized (and these figures with them)."""
    assert G["topk_cap"] == 2048, "top-k grid cap: re-size TOPK_CASES['trips']"
    assert (G["attr_cap"], G["attr_per_block"]) == (4096, 4), "attribution grid: re-size ATTR_CASES['trips']"
    assert (G["weg_cap"], G["weg_per_block"]) == (8192, 4), "word-gradient grid: re-size WEG_CASES['trips']"
    assert (G["gather_cap"], G["gather_per_block"]) == (1024, 256), "gather grid: re-size MOVER_TRIPS"
    assert (G["scatter_cap"], G["scatter_per_block"]) == (1024, 256), "scatter grid: re-size MOVER_TRIPS"
    assert G["QB"] == 128, "attention_probs QB: re-size PROBS_CASES (grids, the odd grid of 9)"
    assert G["kc_chain"] == [(1, 1), (4, 4), (8, 8), (12, 12), (16, 16)], "top-k instances: re-pick the k of TOPK_CASES"
    assert G["topk_sweep"] == 8192 and G["weg_chunk"] == 512 and G["gather_tile"] == 128 and G["TK"] == 64


# ---- top-k ----------------------------------------------------------------------------------------------------------
def test_topk_trips_case_takes_three_trips_with_different_rows_in_each():
    cap, count, ncols, ld, ks = ar.TOPK_CASES["trips"]
    C = G["topk_cap"]
    assert ar.trips(count, C, 1) >= 3 and count < cap, "TOPK_CASES['trips']"
    assert min(cap, C) == C                                    # the launcher's grid is the cap
    three = [r for r in range(C) if r + 2 * C < count]
    assert len(three) == count - 2 * C == 37
    for r in range(min(count - C, C)):
        rows = [r, r + C] + ([r + 2 * C] if r + 2 * C < count else [])
        kinds = [ar.topk_trip_kind(x) for x in rows]
        assert len({k for k, _ in kinds}) == len(rows) and len({lv for _, lv in kinds}) == len(rows), (r, kinds)
    x, _ = ar.topk_inputs("trips", torch.float32)
    level = x[:count, :ncols].median(1).values
    assert (level[:C] > 10).all() and (level[C:2 * C] < -10).all() and (level[2 * C:].abs() < 5).all()
    assert {ar.kc_of(k) for k in ks} == {1, 4, 8, 12, 16}


def test_topk_k_lists_launch_every_instance_and_both_sides_of_every_boundary():
    ks = ar.TOPK_CASES["instances"][4]
    chain = G["kc_chain"]
    assert {ar.kc_of(k) for k in ks} | {ar.kc_of(1)} == {kc for _, kc in chain}
    assert {ar.kc_of(k) for case in ar.TOPK_CASES.values() for k in case[4]} == {1, 4, 8, 12, 16}
    for (kmax, kc), (_, kc_next) in zip(chain[:-1], chain[1:]):
        assert ar.kc_of(kmax) == kc and ar.kc_of(kmax + 1) == kc_next
        assert kmax + 1 in ks or kmax + 1 in ar.TOPK_CASES["trips"][4] or kmax + 1 in ar.TOPK_CASES["misaligned"][4], kmax + 1
    for kc in (4, 8, 12):
        assert kc in ks                                        # k == KC: the list is full to its last slot
    assert all(k <= 16 for case in ar.TOPK_CASES.values() for k in case[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_topk_special_rows_hold_what_they_are_named_for(dtype):
    cap, count, ncols, ld, ks = ar.TOPK_CASES["special"]
    x, tgt = ar.topk_inputs("special", dtype)
    _, _, kinds = ar.topk_special_rows(ncols)
    body = x[:, :ncols]
    assert (x[:, ncols:] == ar.TOPK_PAD).all() and ld % 8 == 0 and ld > ncols
    by = lambda kind: [r for r, k in kinds.items() if k == kind]
    T = body.gather(1, tgt.long()[:, None])[:, 0]
    for r in by("zeros"):
        z = body[r] == 0
        assert (z & torch.signbit(body[r])).sum() >= 8 and (z & ~torch.signbit(body[r])).sum() >= 8
        assert float(body[r].max()) == 0.0 and T[r] == 0      # the zeros are the row's best, the target is one of them
        first = z.nonzero()[:16, 0]
        assert torch.signbit(body[r][first]).any() and (~torch.signbit(body[r][first])).any()   # both signs among the best 16
    assert any(torch.signbit(T[r]) for r in by("zeros")) and any(not torch.signbit(T[r]) and T[r] == 0 for r in by("zeros"))
    fin = [int(torch.isfinite(body[r]).sum()) for r in by("neg_inf")]
    assert min(fin) >= 16 and 16 in fin and all(f <= 30 for f in fin)
    assert any(T[r] == ar.NEG_INF for r in by("neg_inf")) and any(torch.isfinite(T[r]) for r in by("neg_inf"))
    for r in by("ascending"):
        assert (body[r][1:] > body[r][:-1]).all()
    for r in by("descending"):
        assert (body[r][1:] < body[r][:-1]).all()
    assert len(by("ascending")) >= 1 and len(by("descending")) >= 1
    ext = torch.cat([body[r] for r in by("extremes")])
    assert float(ext.max()) == 65504.0 and float(ext.min()) == -65504.0 and torch.isfinite(ext).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_topk_sweep_and_misaligned_cases(dtype):
    cap, count, ncols, ld, ks = ar.TOPK_CASES["sweep"]
    x, tgt = ar.topk_inputs("sweep", dtype)
    per16 = 16 // x.element_size()
    assert ncols > G["topk_sweep"] and ld % per16 == 0         # read in 16-byte pieces, a second sweep of one piece
    assert (x[0, 1:ncols] > x[0, :ncols - 1]).all() and (x[1, 1:ncols] < x[1, :ncols - 1]).all()
    e = ar.topk_expected("sweep", dtype)
    assert (e["si"][0].long() >= ncols - 16).all() and int(e["si"][0, 0]) == ncols - 1   # the best 16 lie behind the boundary
    assert (e["si"][1].long() == torch.arange(16)).all()
    fin = torch.isfinite(x[3, :ncols]).nonzero()[:, 0]
    assert 16 <= len(fin) < 64 and fin.min() < G["topk_sweep"] <= fin.max()
    cap, count, ncols, ld, ks = ar.TOPK_CASES["misaligned"]
    assert ld % 8 == 0                                         # only the base pointer (+ 1 element) forbids the pieces
    a, b = ar.topk_inputs("misaligned", dtype), ar.topk_inputs("instances", dtype)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(ar.TOPK_CASES))
def test_topk_lse_is_away_from_zero_and_targets_are_columns(name, dtype):
    cap, count, ncols, ld, ks = ar.TOPK_CASES[name]
    e = ar.topk_expected(name, dtype)
    x, tgt = ar.topk_inputs(name, dtype)
    assert torch.isfinite(e["lse"]).all() and float(e["lse"].abs().min()) > 1.0   # (a relative bound needs it)
    assert int(tgt.min()) >= 0 and int(tgt.max()) < ncols and ncols >= 16 and count <= cap
    assert x.shape == (cap, ld) and not torch.isnan(x).any()


def _differs(a, b):
    return {k for k in a if not torch.equal(a[k], b[k])}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_topk_references_with_one_mistake_are_told_apart(dtype):
    """The comparison of ids, values, rank and target logit is exact: a mistaken reference must change one of them on the
    case meant for it."""
    cap, count, ncols, ld, ks = ar.TOPK_CASES["special"]
    x, tgt = ar.topk_inputs("special", dtype)
    true = ar.topk_expected("special", dtype)
    assert "si" in _differs(true, ar.topk_reference(x, tgt, count, ncols, "neg_zero_below"))      # -0.0 ordered below +0.0
    assert "si" in _differs(true, ar.topk_reference(x, tgt, count, ncols, "ties_reversed"))
    assert "rank" in _differs(true, ar.topk_reference(x, tgt, count, ncols, "rank_ge"))
    # ... at k = 1 already (the first column of the ids), and on the heavily tied rows of the other cases
    assert not torch.equal(true["si"][:, :1], ar.topk_reference(x, tgt, count, ncols, "neg_zero_below")["si"][:, :1])
    for name in ("trips", "instances"):
        cap, count, ncols, ld, ks = ar.TOPK_CASES[name]
        x, tgt = ar.topk_inputs(name, dtype)
        true = ar.topk_expected(name, dtype)
        assert {"si"} <= _differs(true, ar.topk_reference(x, tgt, count, ncols, "ties_reversed"))
        assert {"rank"} <= _differs(true, ar.topk_reference(x, tgt, count, ncols, "rank_ge"))


def test_topk_reference_orders_by_value_then_column():
    x = torch.tensor([[1.0, -0.0, 3.0, 0.0, 3.0, ar.NEG_INF, 1.0] + [ar.NEG_INF] * 9])
    e = ar.topk_reference(x, torch.tensor([3], dtype=torch.int32), 1, 16)
    assert e["si"][0, :5].tolist() == [2, 4, 0, 6, 1] and int(e["si"][0, 5]) == 3 and int(e["rank"][0]) == 5
    assert abs(float(e["lse"][0]) - math.log(2 * math.e ** 3 + 2 * math.e + 2)) < 1e-12


# ---- input attribution ----------------------------------------------------------------------------------------------
def test_attribution_cases_reach_their_branches():
    c = ar.ATTR_CASES["trips"]
    assert ar.trips(c["B"] * c["S"], G["attr_cap"], G["attr_per_block"]) >= 2, "ATTR_CASES['trips']"
    lanes = lambda H: [min(max(H // 8 - 64 * i, 0), 64) for i in range(-(-H // 512))]   # live lanes per chunk of 64 x 8 columns
    assert lanes(8) == [1] and lanes(72) == [9] and lanes(520) == [64, 1] and lanes(4096) == [64] * 8
    assert {ar.ATTR_CASES[n]["H"] for n in ("H8", "H72", "H520", "H4096")} == {8, 72, 520, 4096}
    assert ar.ATTR_CASES["half0"]["half"] == 0 and ar.ATTR_CASES["halfS"]["half"] == ar.ATTR_CASES["halfS"]["S"]
    for name, c in ar.ATTR_CASES.items():
        i = ar.attr_inputs(name)
        rop = i["row_of_pos"]
        live = rop[rop >= 0]
        assert (live[1:] < live[:-1]).any(), name                        # read rows first: not monotone
        assert sorted(live.tolist()) == list(range(len(live))), name     # a packing: every row once
        assert 0.1 < float((rop < 0).float().mean()) < 0.7, name         # dropped positions: exactly 0 in the packed layout
        assert i["ids"][0, -4:].tolist() == [-1, -(1 << 40), ar.ATTR_KG_ROWS, ar.ATTR_KG_ROWS - 1]
        assert (rop[c["S"] - 4:c["S"]] >= 0).all(), name                 # the out-of-table ids sit on kept positions
        r = ar.attr_reference(name, "packed")
        if c["half"] < c["S"]:
            bad = slice(c["S"] - 4, c["S"] - 1)
            assert (r["gxi"][bad] == 0).all() and (r["gn"][bad] > 0).all() and r["gxi"][c["S"] - 1] != 0
        assert (r["g"][~r["live"]] == 0).all()


# ---- attention probabilities ----------------------------------------------------------------------------------------
def test_probability_cases_reach_their_branches():
    S = {n: c["S"] for n, c in ar.PROBS_CASES.items()}
    assert S["s1024"] > 512 and S["s4096"] == G["probs_max_S"]
    grids = {n: c["B"] * c["NH"] * (c["S"] // G["QB"]) for n, c in ar.PROBS_CASES.items()}
    assert grids["grid9"] == 9 and grids["grid9"] % 8 != 0                # xcd_linear with a remainder
    assert {c["scale"] for c in ar.PROBS_CASES.values()} == {0.125, 0.2}
    assert {ar.PROBS_CASES["grid9"]["half"], ar.PROBS_CASES["s1024"]["half"]} == {64, 192}
    for name, c in ar.PROBS_CASES.items():
        assert c["half"] % G["TK"] == 0 and 0 < c["half"] < c["S"] and c["S"] % G["QB"] == 0
        assert (ar.probs_inputs(name)["key_mask"].sum(1) > 0).all()      # (the reference's -inf needs a live key)
    m = ar.probs_inputs("grid9-sparse")["key_mask"]
    tk, s = G["TK"], S["grid9-sparse"]
    assert m[0].sum() == 1 and m[0, ar.ONE_LIVE_KEY] == 1
    assert m[1, :s - tk].sum() == 0 and m[1, s - tk:].sum() >= 16
    assert m[2, tk:].sum() == 0 and m[2, :tk].sum() >= 16


@pytest.mark.parametrize("name", list(ar.PROBS_CASES))
def test_probability_references(name):
    c = ar.probs_inputs(name)
    (p64, m64), (p32, m32) = ar.probs_expected(name)
    live = (c["key_mask"] != 0)[:, None, None, :].expand_as(p64)
    assert (p64[~live] == 0).all() and float((p64.sum(-1) - 1).abs().max()) < 1e-12
    assert float((m64.sum(-1) - 1).abs().max()) < 1e-12
    if c["mask"] == "sparse":      # the relative bound is about the live keys here; the masked ones are compared exactly
        assert float((p64[live] > ar.PROBS_FLOOR).float().mean()) >= 0.5
        one = p64[0]
        assert (one[..., ar.ONE_LIVE_KEY] == 1.0).all() and one.sum() == one.shape[0] * one.shape[1]   # exactly 1.0 and 0.0
        assert (p32[0] == one.float()).all()
        assert (m64[0, ..., 1] == 1.0).all() and (m64[0, ..., 0] == 0.0).all()                           # key 200 >= half
        assert (m64[1, ..., 0] == 0.0).all() and (m64[2, ..., 1] == 0.0).all()
    else:
        assert float((p64 > ar.PROBS_FLOOR).float().mean()) >= 0.5
    e32, a = pu.tol_a(p32, p64)
    rel32 = ar.probs_rel(p32, p64)
    print(f"{name}: e32 {e32:.3e} A {a:.3e}, r32 relative {rel32:.3e}, relative bound {ar.PROBS_REL_FACTOR * rel32:.3e}")
    assert ar.PROBS_REL_FACTOR * rel32 < 5e-4                              # (an order below the 5e-3 this replaces)
    # another log2(e): the scores scaled by 1.4427 / log2(e)
    pm, mm = ar.probs_reference(name, torch.float64, score_factor=1.4427 * math.log(2.0))
    assert float((pm - p64).abs().max()) > a and ar.probs_rel(pm, p64) > ar.PROBS_REL_FACTOR * rel32, name
    # the masses split one key tile further on
    _, ms = ar.probs_reference(name, torch.float64, split=c["half"] + 64)
    _, am = pu.tol_a(m32, m64)
    assert float((ms - m64).abs().max()) > 100 * am, name      # (grid9-sparse: key 200 changes sides, a mass goes from 1 to 0)


# ---- word-embedding gradient ----------------------------------------------------------------------------------------
def test_word_gradient_cases_reach_their_branches():
    c = ar.WEG_CASES["trips"]
    assert ar.trips(c["B"] * c["S"], G["weg_cap"], G["weg_per_block"]) >= 2, "WEG_CASES['trips']"
    chunk = G["weg_chunk"]
    assert 72 % 64 != 0 and 72 < chunk                                   # `col < H` inside a group of 64 lanes
    assert 520 - chunk == 8                                              # the second chunk: one live lane of 8 columns
    assert 1024 == 2 * chunk
    assert {ar.WEG_CASES[n]["H"] for n in ("H72", "H520", "H1024")} == {72, 520, 1024}
    for name in ar.WEG_CASES:
        for packed in (False, True):
            i = ar.weg_inputs(name, packed)
            ref, mag, count = ar.weg_reference(i, 0)
            assert count[ar.WEG_HOT] >= ar.WEG_N_HOT * 0.5 and count[i["vocab"] - 1] >= 1 and count[0] == 0
            assert ar.weg_reference(i, -1)[2][0] >= 6
            last = i["B"] * i["S"] - 1                                   # the last position is live and in the second trip
            assert int(i["ids"].reshape(-1)[last]) == i["vocab"] - 1 and (not packed or i["row_of_pos"][last] >= 0)


# ---- row movers -----------------------------------------------------------------------------------------------------
def test_mover_cases_reach_their_branches():
    t = ar.MOVER_TRIPS
    nch = t["cols"] // 8
    per_trip = G["gather_cap"] * G["gather_per_block"]
    lim = ar.gather_lim(t["count"], t["cap"])
    assert lim == t["cap"] and lim * nch > per_trip, "MOVER_TRIPS (gather)"
    assert t["count"] * nch > G["scatter_cap"] * G["scatter_per_block"], "MOVER_TRIPS (scatter)"
    assert per_trip // nch < t["count"] < lim                             # moved AND zero-filled rows in the second trip
    assert len({t["cols"], t["ld_src"], t["ld_dst"]}) == 3 and t["ld_src"] % 8 == 0 and t["ld_dst"] % 8 == 0
    s = ar.MOVER_SMALL
    assert len({s["cols"], s["ld_src"], s["ld_dst"]}) == 3
    lims = {(n, cap): ar.gather_lim(n, cap) for n in ar.MOVER_COUNTS for cap in ar.MOVER_CAPS}
    assert lims[(0, 190)] == 0 and lims[(128, 190)] == 128                # nothing / no zero-filled row at all
    assert lims[(190, 190)] == 190 and lims[(190, 200)] == 200 and lims[(190, 256)] == 256   # cap inside / at the tile's end
    src = torch.arange(6 * 8, dtype=torch.float32).view(6, 8)
    rows = torch.tensor([4, 0, 5, 2], dtype=torch.int32)
    out = ar.gather_reference(src, rows, 2, 3, 5, 8)
    assert torch.equal(out[:2].float(), src[[4, 0]]) and (out[2] == 0).all() and (out[3:] == ar.MOVER_FILL).all()
    back = ar.scatter_reference(src, rows, 3, 6, 8)
    assert torch.equal(back[[4, 0, 5]].float(), src[:3]) and (back[[1, 2, 3]] == ar.MOVER_FILL).all()


def test_label_compaction_cases():
    B, half, S, frac = ar.COMPACT_CASES["chunks"]
    assert B * half > G["compact_chunk"] and (B * half) % G["compact_chunk"] != 0
    assert ar.COMPACT_CASES["short"][0] * ar.COMPACT_CASES["short"][1] < 1024
    for name, (B, half, S, frac) in ar.COMPACT_CASES.items():
        assert S > 2 * half                                              # b * S is not b * 2 half: the stride shows
        labels, row_map = ar.compact_labels(name)
        r0, t0 = ar.compact_reference(labels, half, S, 0)
        rh, th = ar.compact_reference(labels, half, S, half)
        assert torch.equal(t0, th) and torch.equal(rh, r0 + half) and len(r0) > 100   # an ignored offset shows in every row
        rm, _ = ar.compact_reference(labels, half, S, 0, row_map)
        assert not torch.equal(rm, r0) and int(rh.max()) < B * S
