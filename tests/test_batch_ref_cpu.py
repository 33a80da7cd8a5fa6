"""CPU (no GPU): tests/batch_ref.py proves its cases. Every case of tests/test_batch_parity_gpu.py reaches the branch it is
there for - decided by constants read out of the launchers' source lines, so an edited launcher fails here by name -, the
kernel-shaped models equal the restatement (oracle/masking_oracle.py) on every case, the invariants hold of them, and a
model with ONE mistake differs from the restatement in at least one element of a case named here. Integer work: every
comparison is equality. Two of the listed mistakes CANNOT differ from the true kernel on any input; the tests say why
instead of pretending. The refused and empty calls of the three launchers return before any launch."""
import numpy as np
import pytest

from oracle import masking_oracle as mo
from stonkgs_amd import _hip
from tests import batch_ref as br


# ------------------------------------------------------------------------------------------------ geometry
def test_launch_constants_are_the_ones_the_cases_were_sized_for():
    g = br.geometry()
    assert g == dict(tpb=256, ws_per_seq=3, mask_block=64, mask_half_limit=8192, assemble_block=256)
    assert _hip.lib().stonk_unpad_workspace_ints(7) == g["ws_per_seq"] * 7 and _hip.lib().stonk_unpad_workspace_ints(0) == 0


# ------------------------------------------------------------------------------------------------ the threshold finding
def test_negative_threshold_is_the_one_of_the_abis_float():
    """stonk_assemble_rows takes `negative_rate` as a C float and stonk_drop_thr32 computes (double)(float)p * 2^32 + 0.5:
    the restatement used the Python double. The two thresholds, and seeds constructed by running the stream backwards so
    that row 1's draw lies between them."""
    assert (br.thr_float(0.2), br.thr_double(0.2)) == (858993472, 858993459)
    assert br.thr_float(0.1) - br.thr_double(0.1) == 6 and br.thr_float(0.999999) - br.thr_double(0.999999) == -57
    assert br.thr_float(0.0) == 0 and br.thr_float(0.5) == 1 << 31 == br.thr_double(0.5)
    assert mo.drop_thr32(1.0) == 0xFFFFFFFF and mo.drop_thr32(-1.0) == 0             # (the clamps)
    for x in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert br.unh32(br.h32(x)) == x and br.h32(x) == int(mo.hash32(x)) and br.base_key(x) == int(mo.base_key(x))
    for rate, seed in br.GAP_SEEDS.items():
        got, draw, lo, hi = br.gap_seed(rate)
        assert got == seed and lo < hi and lo <= draw < hi and br.neg_draw(seed, 1) == draw
        assert (draw < br.thr_float(rate)) != (draw < br.thr_double(rate))
    assert br.gap_seed(0.2)[1] == 858993465


def test_the_old_threshold_rule_fails_on_the_gap_seeds():
    for name, rate, kernel_says_negative in (("gap_02", 0.2, 1), ("gap_01", 0.1, 1), ("gap_1", 0.999999, 0)):
        c = br.assemble_cases()[name]
        assert c["rate"] == rate and c["seed"] == br.GAP_SEEDS[rate]
        want, old = br.assemble_expected(name), br.assemble_model(c, wrong="thr_double")
        assert want[3][1] == kernel_says_negative and old[3][1] == 1 - kernel_says_negative
        assert not np.array_equal(want[0][1], old[0][1])                            # (row 1's entity half differs too)
        assert br.same_arrays(br.assemble_model(c), want)


# ------------------------------------------------------------------------------------------------ row plan
def test_restatement_default_half_is_unchanged_and_other_halves_follow_the_rule():
    """half=None is S // 2, array for array; the other halves against a hand-made example."""
    c = br.plan_cases()["s64"]
    assert br.same_plan(mo.unpad_plan(c["am"], c["tl"], c["el"], read=True),
                        mo.unpad_plan(c["am"], c["tl"], c["el"], read=True, half=32))
    am = np.array([[0, 3, 0, 0, 0, 0, 0]], dtype=np.int64)                            # S 7 (odd), half 2: 2 half < S
    tl, el = np.array([[-100, 5]]), np.array([[-1, -100]])
    rop, por, cu, rm, rr, rofp, ro = mo.unpad_plan(am, tl, el, read=True, half=2)
    assert por[:3].tolist() == [0, 1, 2] and cu.tolist() == [0, 3] and rm[:3].tolist() == [0, 3, 0] and ro.tolist() == [0, 3]
    am2 = am.copy()
    am2[0, 5] = 1 << 40                                                             # kept by its mask word alone
    rop, por, cu, rm, *_ = mo.unpad_plan(am2, tl, el, read=True, half=2)
    assert por[:4].tolist() == [0, 1, 2, 5] and rm[3] == 1 << 40
    rop, por, cu, *_ = mo.unpad_plan(am, None, np.full((1, 9), 4), read=True, half=0)  # half 0: no label is read
    assert cu.tolist() == [0, 2] and por[:2].tolist() == [0, 1]
    rop, por, cu, *_ = mo.unpad_plan(am, np.array([[-100, -100, -100, -100, -100, -100, 8]]), None, half=7)   # half = S
    assert cu.tolist() == [0, 3] and por[:3].tolist() == [0, 6, 1]


def test_plan_cases_reach_their_branches():
    f = {name: br.plan_facts(name) for name in br.plan_cases()}
    cases = br.plan_cases()
    assert (f["s6"]["per"], f["s6"]["idle"]) == (1, 250) and (f["s64"]["per"], f["s64"]["idle"]) == (1, 192)
    assert (f["s255"]["per"], f["s255"]["idle"]) == (1, 1)
    assert (f["s257"]["per"], f["s257"]["last_thread"], f["s257"]["last_held"], f["s257"]["idle"]) == (2, 128, 1, 127)
    assert (f["s1000"]["per"], f["s1000"]["idle"], f["s1000"]["beyond"]) == (4, 6, 5)
    assert (f["s4096"]["per"], f["s4096"]["idle"]) == (16, 0)
    assert [f[n]["count_trips"] for n in ("b1", "b257", "b600")] == [1, 2, 3] and cases["b1"]["am"].shape[0] == 1
    assert [f[n]["live_trips"] for n in ("s255", "s257", "last_key", "s4096")] == [1, 2, 2, 16]
    for name in ("half0_null", "half0_ent"):
        assert cases[name]["half"] == 0 and cases[name]["tl"] is None
    assert cases["half0_null"]["el"] is None and (cases["half0_ent"]["el"] != -100).all()
    assert cases["half_S"]["half"] == cases["half_S"]["am"].shape[1] and (cases["half_S"]["el"] != -100).all()
    assert cases["s255"]["am"].shape[1] % 2 == 1 and cases["s257"]["am"].shape[1] % 2 == 1
    c = cases["s260_h256"]
    assert (c["el"][0, [1, 3, 4, 200]] != -100).all() and (c["am"][0, [257, 259]] == 0).all()
    kept, rd = br.plan_rule(c)
    assert rd[0, 257] and rd[0, 259] and not rd[0, 258]
    c = cases["s512_h100"]
    kept, rd = br.plan_rule(c)
    assert c["am"][0, 300] == 2 and kept[0, 300] and not rd[0, 300] and not kept[0, 200] and c["el"][1, 0] != -100
    assert (cases["text_only"]["tl"] is not None, cases["text_only"]["el"]) == (True, None)
    assert (cases["ent_only"]["tl"], cases["ent_only"]["el"] is not None) == (None, True)
    assert cases["neither"]["tl"] is None and cases["neither"]["el"] is None
    c = cases["s64"]                                                   # a label at position 0, the values -1 and 1 << 40
    assert c["tl"][0, 0] != -100 and c["tl"][0, 31] == -1 and c["el"][1, 0] == 1 << 40
    assert br.plan_rule(c)[1][0, 31] and br.plan_rule(c)[1][1, 32]
    words = set(np.unique(cases["s4096"]["am"]).tolist())
    assert words == {0, 1, 2, -1, 1 << 40}
    for name, pos in (("last_key", 499), ("first_key", 0)):
        live = np.flatnonzero((cases[name]["am"] != 0).any(axis=0))
        assert live.tolist() == [pos]
    tpb = br.geometry()["tpb"]                                       # position 499: second trip, thread 243, the last wave
    assert 499 // tpb == 1 and (499 % tpb) // 64 == tpb // 64 - 1 and cases["last_key"]["am"].shape[1] == 500
    assert not cases["all_dead"]["am"].any() and f["all_dead"]["total"] == 600
    assert (cases["all_live"]["am"] != 0).all() and f["all_live"]["total"] == 600 and f["all_live"]["tail_trips"] == 0
    assert f["tail_fill"]["total"] == 3 and f["tail_fill"]["tail_trips"] == 16
    c = cases["dead_labels"]
    assert not c["am"][1].any() and c["am"][0].any() and c["am"][2].any() and br.plan_rule(c)[0][1].all()
    want, n_rd = br.plan_expected("dead_labels"), int(br.plan_rule(c)[1][1].sum())
    first = want[1][want[2][1]:want[2][2]] - 64                    # sequence 1's positions, in packed order
    assert n_rd >= 4 and len(first) == 64 and first[0] == 0 and {3, 9, 32 + 5} <= set(first[:n_rd].tolist())
    assert first[n_rd] < first[n_rd - 1]                           # (the other rows start over from the front)


@pytest.mark.parametrize("name", sorted(br.plan_cases()))
def test_plan_model_equals_the_restatement_and_the_invariants_hold(name):
    c = br.plan_cases()[name]
    want, model = br.plan_expected(name), br.plan_model(c)
    for key, a, b in zip(br.PLAN_NAMES, model, want):
        assert np.array_equal(a, b), key
    assert br.plan_invariants(c, want, read=True) == br.plan_invariants(c, want[:4], read=False) == int(want[2][-1])


# mistake -> cases that must tell it apart (row_of_pos and friends differ from the restatement, and the invariants fail)
PLAN_TOLD_APART = {
    "ent_le": ("s512_h100",),
    "read_not_first": ("s64", "dead_labels", "s4096"),
    "live_first_block": ("last_key",),
    "floor_chunk": ("s6", "s257", "s1000"),
    "prefix_le": ("s6", "b257", "b600"),
}


def test_plan_mistakes_are_told_apart_by_named_cases():
    assert set(PLAN_TOLD_APART) == set(br.PLAN_WRONG)
    for wrong, names in PLAN_TOLD_APART.items():
        for name in names:
            c = br.plan_cases()[name]
            bad = br.plan_model(c, wrong=wrong)
            assert not br.same_plan(bad, br.plan_expected(name), read=False), (wrong, name)
            with pytest.raises(AssertionError):
                br.plan_invariants(c, bad, read=True)
    # the mistakes that need their branch leave the cases without it alone: the cases above are not told apart by accident
    assert br.same_plan(br.plan_model(br.plan_cases()["s64"], wrong="live_first_block"), br.plan_expected("s64"))
    assert br.same_plan(br.plan_model(br.plan_cases()["s4096"], wrong="floor_chunk"), br.plan_expected("s4096"))
    assert br.same_plan(br.plan_model(br.plan_cases()["s260_h256"], wrong="ent_le"), br.plan_expected("s260_h256"))
    assert br.same_plan(br.plan_model(br.plan_cases()["neither"], wrong="read_not_first")[:4],
                        br.plan_expected("neither")[:4], read=False)        # (no labels: position 0, the only read row, is first anyway)


# ------------------------------------------------------------------------------------------------ masking
def test_mask_cases_reach_their_branches():
    g, cases = br.geometry(), br.mask_cases()
    assert [cases[n]["half"] for n in ("h1", "h2_b1000", "h63", "h65", "h100", "h8192")] == [1, 2, 63, 65, 100, g["mask_half_limit"]]
    assert all(cases[n]["half"] % g["mask_block"] for n in ("h1", "h2_b1000", "h63", "h65", "h100"))
    assert -(-65 // g["mask_block"]) == 2 and -(-63 // g["mask_block"]) == 1 and g["mask_half_limit"] // g["mask_block"] == 128
    assert cases["h8192"]["half"] * 4 == 32768 and cases["h8192"]["ids"].shape == (1, 16384)
    assert cases["h2_b1000"]["ids"].shape[0] == 1000
    ks = {(c["k_text"], c["k_ent"], c["half"]) for c in cases.values()}
    assert any(kt == 0 or ke == 0 for kt, ke, _ in ks) and any(kt == h or ke == h for kt, ke, h in ks)
    assert all(c["k_text"] != c["k_ent"] for c in cases.values())
    assert {cases["h63"]["vocab_text"], cases["h63"]["vocab_ent"]} == {1, (1 << 32) - 1}
    assert cases["h63"]["mask_id"] < 0 and cases["h100"]["mask_id"] > 1 << 31
    assert cases["h100"]["ids"].min() > 1 << 32 and {cases["h1"]["seed"], cases["h100"]["seed"]} == {0, 0xFFFFFFFF}
    out = br.mask_expected("h63")[0]
    assert out[:, 63:].max() > 1 << 31 and ((out[:, 63:] >= 0) & (out[:, 63:] < 1 << 32) & (out[:, 63:] != 0)).any()


def test_mask_keys_never_tie():
    """key(pos) = lowbias32(rowkey + pos * K_POS): K_POS is odd, so pos -> pos * K_POS is a bijection of 32-bit words, and
    so are the addition of a constant and lowbias32 - two positions below 2^32 never share a key, in any half, for any seed.
    A rank tie-break that ignores the position therefore CANNOT differ from the kernel's; the mistake is listed and its
    model is run, and it equals the restatement."""
    assert mo.K_POS % 2 == 1
    for name, c in br.mask_cases().items():
        keys = br.mask_keys(c, 0, 1)
        assert len(np.unique(keys)) == c["half"], name
    for name in ("h63", "h65", "h100"):
        assert br.same_arrays(br.mask_model(br.mask_cases()[name], wrong="tie_ignores_position"), br.mask_expected(name))


@pytest.mark.parametrize("name", sorted(br.mask_cases()))
def test_mask_model_equals_the_restatement_and_the_invariants_hold(name):
    c = br.mask_cases()[name]
    want = br.mask_expected(name)
    assert br.same_arrays(br.mask_model(c), want)
    br.mask_invariants(c, want)


MASK_TOLD_APART = {"rank_le": ("h1", "h63", "h100"), "keep_random_swapped": ("h65", "h100", "h8192")}


def test_mask_mistakes_are_told_apart_by_named_cases():
    assert set(MASK_TOLD_APART) | {"tie_ignores_position"} == set(br.MASK_WRONG)
    for wrong, names in MASK_TOLD_APART.items():
        for name in names:
            c = br.mask_cases()[name]
            assert not br.same_arrays(br.mask_model(c, wrong=wrong), br.mask_expected(name)), (wrong, name)
    for name in MASK_TOLD_APART["rank_le"]:                       # (one label too many: the invariants see it alone)
        with pytest.raises(AssertionError):
            br.mask_invariants(br.mask_cases()[name], br.mask_model(br.mask_cases()[name], wrong="rank_le"))


# ------------------------------------------------------------------------------------------------ assembly
def test_assemble_cases_reach_their_branches():
    g, cases = br.geometry(), br.assemble_cases()
    assert br.find_fallback_seed(2) == br.FALLBACK_SEEDS[2] and br.find_fallback_seed(3) == br.FALLBACK_SEEDS[3]
    for name, B in (("fallback_b2", 2), ("fallback_b3", 3)):
        rows = br.assemble_rows_of(cases[name])
        hit = [b for b, (neg, drawn, used) in enumerate(rows) if neg and drawn == b]
        assert hit and all(rows[b][2] == (b + 1) % B for b in hit) and cases[name]["text"].shape[0] == B
    assert br.assemble_rows_of(cases["b1"]) == [(False, 0, 0)] and cases["b1"]["rate"] == 0.99
    assert not any(neg for neg, _, _ in br.assemble_rows_of(cases["rate0"]))
    assert br.find_partner_only_seed() == br.PARTNER_ONLY_SEED
    r, readers = br.partner_only_rows()
    c = cases["bad_partner"]
    rows = br.assemble_rows_of(c)
    assert c["source"][r] == 40 == c["walks"].shape[0] and rows[r][0] and rows[r][2] != r            # r never reads itself
    assert readers and all(rows[b][0] and rows[b][2] == r for b in readers)
    assert [b for b in range(3) if rows[b][2] == r] == readers
    assert cases["bad_source"]["source"][1] == 40 and cases["bad_target"]["target"][2] == -1
    shapes = {n: cases[n]["text"].shape[0] * 2 * cases[n]["half"] for n in ("h4", "h100", "h128")}
    assert shapes == {"h4": 24, "h100": 600, "h128": 768} and cases["h4"]["walks"].shape[1] == 1
    assert shapes["h4"] % g["assemble_block"] and shapes["h100"] % g["assemble_block"] and shapes["h100"] > 2 * g["assemble_block"]
    for name in ("h4", "h100", "h128"):                             # both kinds of row in the shape cases
        negs = [neg for neg, _, _ in br.assemble_rows_of(cases[name])]
        assert any(negs) and not all(negs), name


@pytest.mark.parametrize("name", sorted(br.assemble_cases()))
def test_assemble_model_equals_the_restatement_and_the_invariants_hold(name):
    c = br.assemble_cases()[name]
    want = br.assemble_expected(name)
    model = br.assemble_model(c)
    assert br.same_arrays(model[:4], want[:4]) and model[4] == want[4] == int(c["bad"])
    if not c["bad"]:
        br.assemble_invariants(c, want)


def test_bad_nodes_write_zeros_exactly_where_the_bad_node_is_read():
    half, W = 8, 3
    for name, which, readers in (("bad_source", 0, [1]), ("bad_target", 1, [2]), ("bad_partner", 0, br.partner_only_rows()[1])):
        c = br.assemble_cases()[name]
        ids, at, ty, nsp, err = br.assemble_expected(name)
        clean = dict(c, source=np.where(c["source"] == 40, 0, c["source"]), target=np.where(c["target"] == -1, 0, c["target"]))
        ref = br.assemble_model(clean)
        assert err == 1 and ref[4] == 0
        zero = np.zeros((3, 2 * half), dtype=bool)
        lo = half + which * (W + 1)
        zero[readers, lo:lo + W] = True
        assert (ids[zero] == 0).all() and np.array_equal(ids[~zero], ref[0][~zero]) and (ref[0][zero] != 0).all()
        assert br.same_arrays((at, ty, nsp), ref[1:4])


ASSEMBLE_TOLD_APART = {"thr_double": ("gap_02", "gap_01", "gap_1"), "fallback_keeps_b": ("fallback_b2", "fallback_b3"),
                       "bad_as_sep": ("bad_source", "bad_target", "bad_partner")}


def test_assemble_mistakes_are_told_apart_by_named_cases():
    """`second_ge` (the target's walk from e >= walk_len on) CANNOT differ: e == walk_len has been given [SEP] before the
    test is reached, on every input. Listed, run, and equal to the restatement."""
    assert set(ASSEMBLE_TOLD_APART) | {"second_ge"} == set(br.ASSEMBLE_WRONG)
    for wrong, names in ASSEMBLE_TOLD_APART.items():
        for name in names:
            c = br.assemble_cases()[name]
            bad = br.assemble_model(c, wrong=wrong)
            assert not br.same_arrays(bad[:4], br.assemble_expected(name)[:4]), (wrong, name)
            if wrong == "fallback_keeps_b":                         # (a threshold is nothing the invariants can know)
                with pytest.raises(AssertionError):
                    br.assemble_invariants(c, bad)
    for name, c in br.assemble_cases().items():
        assert br.same_arrays(br.assemble_model(c, wrong="second_ge")[:4], br.assemble_expected(name)[:4]), name


# ------------------------------------------------------------------------------------------------ refused and empty calls
def test_refused_and_empty_calls_return_before_any_launch():
    """Every check of the three launchers, in its order (the first failing one decides the code: -1 argument, -2 shape),
    and the empty call that returns 0 before anything is launched. P = a non-null address that is never dereferenced."""
    P, lib = 16, _hip.lib()
    plan = lambda am=P, B=2, S=8, half=4, rop=P, ws=P, rd=(P, P, P), ws_ints=6: (
        "stonk_unpad_plan", (am, 0, 0, B, S, half, rop, P, P, P) + rd + (ws, ws_ints, 0))
    mask = lambda out=P, B=2, S=8, half=4, vt=10, ve=10, kt=1, ke=1: (
        "stonk_mlm_mask", (P, out, P, P, B, S, half, vt, ve, 103, kt, ke, 0, 0))
    asm = lambda walks=P, n_nodes=5, W=3, B=2, S=16, half=8, rate=0.2, err=P: (
        "stonk_assemble_rows", (P, P, P, P, walks, n_nodes, W, P, P, P, P, B, S, half, 102, rate, 0, err, 0))
    table = [
        (plan(am=0), -1), (plan(rop=0), -1), (plan(ws=0), -1),                      # null groups
        (plan(rd=(P, 0, 0)), -1), (plan(rd=(P, P, 0)), -1), (plan(rd=(0, 0, P)), -1),   # the read outputs: all or none
        (plan(am=0, half=9), -1),                                                   # (the pointers are looked at first)
        (plan(half=9), -2), (plan(half=-1), -2), (plan(S=0, half=0), -2), (plan(B=-1), -2),
        (plan(B=32768, S=65536, ws_ints=1 << 20), -2),                              # B S = 2^31
        (plan(B=32768, S=65535, ws_ints=3 * 32768 - 1), -1),                        # (one position less: the workspace is next)
        (plan(ws_ints=5), -1),                                                      # ws_ints = 3 B - 1
        (plan(B=0, ws_ints=-1), -1),
        (plan(B=0, ws_ints=0), 0), (plan(B=0, S=7, half=7, rd=(0, 0, 0), ws_ints=0), 0),
        (mask(out=0), -1),
        (mask(S=9), -2), (mask(S=0, half=0), -2), (mask(B=-1), -2),
        (mask(S=16386, half=8193), -2),
        (mask(out=0, S=9), -1),
        (mask(vt=1 << 32), -1), (mask(ve=1 << 32), -1), (mask(vt=0), -1),
        (mask(vt=1 << 32, S=9), -2),                                                # (the shape before the vocabulary)
        (mask(kt=5), -1), (mask(ke=5), -1), (mask(kt=-1), -1),
        (mask(kt=5, vt=0), -1),
        (mask(B=0), 0), (mask(B=0, S=16384, half=8192, kt=8192, ke=0, vt=(1 << 32) - 1), 0),
        (asm(walks=0), -1), (asm(err=0), -1),
        (asm(W=4), -2), (asm(S=17), -2), (asm(n_nodes=0), -2), (asm(B=-1), -2), (asm(S=0, half=0, W=-1), -2),
        (asm(err=0, W=4), -1),
        (asm(rate=1.0), -1), (asm(rate=-0.1), -1),
        (asm(rate=0.99999999), -1),                                                 # (a double below 1 that is 1.0f)
        (asm(rate=1.0, W=4), -2),
        (asm(B=0), 0), (asm(B=0, rate=0.0, S=4, half=2, W=0), 0),
    ]
    got = [(name, args, getattr(lib, name)(*args)) for (name, args), _ in table]
    wrong = [(name, args, code, want) for (name, args, code), (_, want) in zip(got, table) if code != want]
    assert not wrong, wrong
