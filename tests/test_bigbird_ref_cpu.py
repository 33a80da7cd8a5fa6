"""The block-sparse attention reference (tests/bigbird_ref.py) without a GPU: against HuggingFace's own
BigBirdBlockSparseAttention in float64, through its own checks with r16 in a kernel's place, the host-side lists, and the
C ABI's refusals (which happen before any launch)."""
import numpy as np
import pytest
import torch

from stonkgs_amd import _hip
from stonkgs_amd import bigbird_attention as bb
from tests import bigbird_ref as br


# ------------------------------------------------------------------ the list semantics ARE HuggingFace's
def _hf_case(S, mode, inject):
    from transformers.models.big_bird.modeling_big_bird import BigBirdBlockSparseAttention, BigBirdConfig, BigBirdModel

    B, NH, H, nb = 2, 2, 128, S // 64
    cfg = BigBirdConfig(hidden_size=H, num_attention_heads=NH, attention_type="block_sparse", block_size=64,
                        num_random_blocks=3, max_position_embeddings=4096, use_bias=True)
    torch.manual_seed(S)
    attn = BigBirdBlockSparseAttention(cfg, seed=0).double()
    attn.train(mode == "train")
    ra = bb.bigbird_rand_attn(nb, 3, NH, mode, seed=21)
    if inject:   # the plan, through the instance's two rand-mask methods
        calls = [0]

        def per_head(*a, **k):      # (called once per head at 1024 / 3072 / 4096 tokens; the caller cuts it to nb - 2 rows)
            calls[0] += 1
            return ra[(calls[0] - 1) % NH]

        attn._bigbird_block_rand_mask = per_head
        attn._bigbird_block_rand_mask_with_head = lambda *a, **k: [ra[h] for h in range(NH)]
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, 70:90] = 0
    mask[1, S - 100:] = 0     # the whole last block, a global one
    x = torch.randn(B, S, H, dtype=torch.float64, generator=torch.Generator().manual_seed(S + 1))
    blocked, band, from_mask, to_mask = BigBirdModel.create_masks_for_block_sparse_attn(mask.double(), 64)
    with torch.no_grad():
        hf = attn(x, band, from_mask, to_mask, blocked, blocked)
        hf = hf[0] if isinstance(hf, tuple) else hf
        qkv = torch.cat([attn.query(x), attn.key(x), attn.value(x)], -1).view(B * S, 3 * H)
    c = dict(B=B, NH=NH, S=S, nb=nb, T=B * S, scale=0.125, mask=mask)
    ref = br.compute(c, bb.bigbird_block_lists(nb, ra), qkv, torch.zeros(B * S, H, dtype=torch.float64), "r64")
    return hf.reshape(B * S, H), ref["out"], mask.view(-1) != 0


@pytest.mark.parametrize("S,mode,inject", [(768, "eval", True), (768, "train", True), (1024, "eval", False)])
def test_list_semantics_are_huggingfaces_on_live_query_rows(S, mode, inject):
    """float64, hidden 128, 2 heads, B = 2, one sequence masked in [70, 90) and in its last 100 positions. At 1024 tokens in
    eval mode nothing is injected: HuggingFace's own plan is the zeros plan."""
    hf, ref, live = _hf_case(S, mode, inject)
    left_out = 1.0 - float(live.double().mean())
    assert int((~live).sum()) == 120 and left_out < 0.10     # exactly the masked queries: the comparison cannot shrink
    err = float((hf[live] - ref[live]).abs().max())
    print(f"HF-AGREEMENT S={S} {mode}: max |hf - r| on {int(live.sum())} live query rows = {err:.2e}; "
          f"on the {int((~live).sum())} masked ones {float((hf[~live] - ref[~live]).abs().max()):.2e}")
    assert err <= 1e-12


# ------------------------------------------------------------------ the checks are satisfiable, and refuse errors
@pytest.mark.parametrize("name", list(br.CASES))
def test_r16_satisfies_every_assertion(name):
    br.check_case(name, br.r16_as_kernel_output(name))


def test_cases_cover_what_they_are_meant_to():
    c = br.CASES
    assert list(c) == ["s384-drawn", "s384-mask", "s320-r1", "s768-eval", "s384-nokey", "s384-r0", "s4096-eval", "s4096-drawn",
                       "exact-s512-drawn", "exact-s512-eval"]
    ra = br.plan("s384-drawn").lists
    assert not np.array_equal(ra["key_mult"][0], ra["key_mult"][1])              # differing per head
    assert not bool(c["s384-mask"]["mask"][1, -64:].any()) and bool(c["s384-mask"]["mask"][0].all())
    assert not bool(c["s384-nokey"]["mask"][0].any()) and bool(c["s384-nokey"]["mask"][1].any())
    cmp = br.lse_compared(c["s384-nokey"], br.plan("s384-nokey").lists)
    assert not bool(cmp[0].any()) and bool(cmp[1].all())
    assert c["s320-r1"]["nb"] == 5 and c["s4096-eval"]["nb"] == 64
    assert [int(n) for n in br.plan("s384-r0").lists["key_count"][0]] == [6, 4, 5, 5, 4, 6]
    assert int(c["s4096-drawn"]["mask"][0].sum()) == 4096 - 1000
    for name in ("exact-s512-drawn", "exact-s512-eval"):     # total multiplicity: 8 on the global and middle rows, 7 on rows 1, nb-2
        L = (br.plan(name).lists["key_mult"].sum(-1))
        assert [int(v) for v in L[0]] == [8, 7, 8, 8, 8, 8, 7, 8]


def test_check_refuses_localised_errors():
    """Each of the issue's four mutations, made on r16's output, and three local slips: every one must fail the check."""
    name = "s384-mask"
    c = br.CASES[name]
    H, S, nb = c["NH"] * 64, c["S"], c["nb"]
    lists = br.plan(name).lists
    qkv, dout = br.inputs(name)

    def refused(got):
        with pytest.raises(AssertionError):
            br.check_case(name, got)

    def mutated(edit):
        l2 = {k: v.copy() for k, v in lists.items()}
        edit(l2)
        r = br.compute(c, l2, qkv, dout, "r16")
        return dict(out=r["out"].to(torch.bfloat16), lse=r["lse"].clone(),
                    dqkv=torch.cat([r["dq"], r["dk"], r["dv"]], 1).to(torch.bfloat16))

    good = br.r16_as_kernel_output(name)
    # multiplicity ignored in the forward (and with it everywhere)
    assert int(lists["key_mult"].max()) >= 2
    refused(mutated(lambda l: l["key_mult"].__setitem__(l["key_mult"] > 1, 1)))
    # multiplicity ignored in dK / dV only: dk, dv of a block listed twice lose that part
    bad = {k: v.clone() for k, v in good.items()}
    once = br.compute(c, {**lists, "key_mult": np.where(lists["key_mult"] > 1, 1, lists["key_mult"])}, qkv, dout, "r16")
    bad["dqkv"][:, H:] = torch.cat([once["dk"], once["dv"]], 1).to(torch.bfloat16)
    refused(bad)

    def window(l):       # block nb-2 given a middle block's window {nb-3, nb-2, nb-1, 0, nb-1}: block nb-1 counts twice
        for hh in range(c["NH"]):
            e = [j for j, _ in br.entries(l, "key", hh, nb - 2)].index(nb - 1)
            l["key_mult"][hh, nb - 2, e] += 1

    refused(mutated(window))
    # random part dropped from the inverse lists: dk / dv without the random blocks' part
    fixed = bb.bigbird_block_lists(nb, bb.bigbird_rand_attn(nb, 0, c["NH"], "eval"))
    nor = br.compute(c, fixed, qkv, dout, "r16")
    bad = {k: v.clone() for k, v in good.items()}
    bad["dqkv"][:, H:] = torch.cat([nor["dk"], nor["dv"]], 1).to(torch.bfloat16)
    refused(bad)
    # local slips
    for edit in (lambda g: g["dqkv"].__setitem__((S + 5, slice(0, 64)), g["dqkv"][S + 6, :64]),
                 lambda g: g["dqkv"].__setitem__((S + 3, slice(2 * H, 2 * H + 64)), 0),
                 lambda g: g["lse"].__setitem__((1, 0, 7), float("nan"))):
        bad = {k: v.clone() for k, v in good.items()}
        edit(bad)
        refused(bad)


# ------------------------------------------------------------------ the lists
@pytest.mark.parametrize("nb,r,mode", [(5, 1, "train"), (6, 3, "train"), (12, 3, "train"), (16, 3, "eval"), (64, 3, "eval"),
                                       (64, 8, "train"), (8, 0, "train")])
def test_forward_and_inverse_lists_are_the_same_multiset(nb, r, mode):
    ra = bb.bigbird_rand_attn(nb, r, 3, mode, seed=nb)
    l = bb.bigbird_block_lists(nb, ra)
    assert all(l[k].dtype == np.int32 for k in l)
    for h in range(3):
        fwd = sorted((i, j, m) for i in range(nb) for j, m in br.entries(l, "key", h, i))
        inv = sorted((i, j, m) for j in range(nb) for i, m in br.entries(l, "query", h, j))
        assert fwd == inv
        # ... and that multiset is the table of the issue: fixed blocks once each, plus rand_attn's, duplicates adding
        want = {}
        for i in range(nb):
            fixed = [0, 1, 2, nb - 1] if i == 1 else [0, nb - 3, nb - 2, nb - 1] if i == nb - 2 else [i - 1, i, i + 1, 0, nb - 1]
            blocks = list(range(nb)) if i in (0, nb - 1) else fixed + [int(v) for v in ra[h, i - 1]]
            for j in blocks:
                want[(i, j)] = want.get((i, j), 0) + 1
        assert fwd == sorted((i, j, m) for (i, j), m in want.items())
        for i in range(nb):      # ascending, no duplicates, zero past the count
            js = [j for j, _ in br.entries(l, "key", h, i)]
            assert js == sorted(set(js)) and not l["key_mult"][h, i, len(js):].any()
        if mode == "train" and nb >= 6 + r:     # distinct, outside the fixed set
            for i in range(1, nb - 1):
                assert len(set(ra[h, i - 1])) == r and not set(ra[h, i - 1]) & set(bb._fixed_blocks(i, nb))


def test_eval_plan_puts_multiplicity_on_block_zero():
    for nb, r in ((16, 3), (64, 3), (12, 2)):
        ra = bb.bigbird_rand_attn(nb, r, 2, "eval")
        assert ra.shape == (2, nb - 2, r) and not ra.any()
        l = bb.bigbird_block_lists(nb, ra)
        for i in range(1, nb - 1):
            ent = dict(br.entries(l, "key", 0, i))
            assert ent[0] == 1 + r
            if 2 <= i <= nb - 3:
                assert len(ent) == 5 and all(m == 1 for j, m in ent.items() if j != 0)
        assert int(l["key_count"][0].sum()) == 2 * nb + 4 * 2 + 5 * (nb - 4)
    assert np.array_equal(bb.bigbird_rand_attn(8, 3, 2, "train", seed=4), bb.bigbird_rand_attn(8, 3, 2, "train", seed=4))
    assert not np.array_equal(bb.bigbird_rand_attn(8, 3, 2, "train", seed=4), bb.bigbird_rand_attn(8, 3, 2, "train", seed=5))


def test_invalid_rand_attn_raises():
    good = bb.bigbird_rand_attn(8, 3, 2, "train", seed=1)
    bb.bigbird_block_lists(8, good)
    for bad in (good[:, :5], good[0], good.astype(np.float32), np.where(good == good.max(), 8, good), good - 8,
                np.zeros((2, 6, 9), dtype=np.int32)):
        with pytest.raises(ValueError):
            bb.bigbird_block_lists(8, bad)
    for nb in (4, 65, 7.5):
        with pytest.raises(ValueError):
            bb.bigbird_block_lists(nb, good)
    with pytest.raises(ValueError):
        bb.bigbird_rand_attn(8, 9, 2, "train")
    with pytest.raises(ValueError):
        bb.bigbird_rand_attn(8, 3, 2, "test")
    with pytest.raises(ValueError):
        bb.BlockSparsePlan.from_lists({**bb.bigbird_block_lists(8, good), "key_mult": np.zeros((2, 8, 7), dtype=np.int32)})


def test_module_raises_without_a_gpu_and_takes_huggingface_keys():
    mod = bb.BigBirdBlockSparseSelfAttention(128, 2)
    assert sorted(mod.state_dict()) == ["key.bias", "key.weight", "query.bias", "query.weight", "value.bias", "value.weight"]
    if not torch.cuda.is_available():
        with pytest.raises(_hip.StonkHipError):
            mod(torch.zeros(1, 384, 128))
    with pytest.raises(ValueError):
        bb.BigBirdBlockSparseSelfAttention(100, 2)


# ------------------------------------------------------------------ the C ABI
FWD, BWD = "stonk_block_sparse_attention_fwd", "stonk_block_sparse_attention_bwd"


def test_abi_exports_and_signatures():
    import ctypes as C

    lib = _hip.lib()
    for name in (FWD, BWD):
        assert name in _hip._SIGNATURES and name in _hip.exported_symbols() and hasattr(lib, name)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert _hip._SIGNATURES[FWD] == [vp] * 3 + [i64] + [vp] * 5 + [i64, vp] + [i32] * 4 + [f32, vp, vp]
    assert _hip._SIGNATURES[BWD] == ([vp] * 3 + [i64] + [vp] * 8 + [i64, vp, i64] + [vp] * 4 + [i64, vp] + [i32] * 4
                                     + [f32, vp, vp])
    header = open(_hip.os.path.join(_hip.os.path.dirname(_hip._HERE), "include", "stonk_hip.h")).read()
    assert f"int {FWD}(" in header and f"int {BWD}(" in header
    assert lib.stonk_abi_version() == 5      # additions: the ABI number stays


def _fwd_args(**kw):
    P = 0x10000      # (never dereferenced: every call below is refused, or returns for B == 0, before any launch)
    a = dict(q=P, k=P + 256, v=P + 512, ld=384, mask=0, kb=P, km=P, kc=P, out=P, ldo=128, lse=P, B=1, NH=2, S=384, D=64, scale=0.125,
             err=P, stream=0)
    a.update(kw)
    return [a[k] for k in ("q", "k", "v", "ld", "mask", "kb", "km", "kc", "out", "ldo", "lse", "B", "NH", "S", "D", "scale", "err",
                           "stream")]


def _bwd_args(**kw):
    P = 0x10000
    a = dict(q=P, k=P + 256, v=P + 512, ld=384, mask=0, kb=P, km=P, kc=P, qb=P, qm=P, qc=P, out=P, ldo=128, dout=P, lddo=128, lse=P,
             ws=P, dq=P, dk=P + 256, ldd=384, dv=P + 512, B=1, NH=2, S=384, D=64, scale=0.125, err=P, stream=0)
    a.update(kw)
    return [a[k] for k in ("q", "k", "v", "ld", "mask", "kb", "km", "kc", "qb", "qm", "qc", "out", "ldo", "dout", "lddo", "lse", "ws",
                           "dq", "dk", "ldd", "dv", "B", "NH", "S", "D", "scale", "err", "stream")]


REFUSALS = [
    (dict(D=32), _hip.ESHAPE), (dict(S=400), _hip.ESHAPE), (dict(S=256), _hip.ESHAPE), (dict(S=4160), _hip.ESHAPE),
    (dict(S=0), _hip.ESHAPE), (dict(NH=0), _hip.ESHAPE), (dict(B=-1), _hip.ESHAPE), (dict(ld=383), _hip.ESHAPE),
    (dict(ld=128), _hip.ESHAPE), (dict(ld=388), _hip.EALIGN), (dict(q=0x10008), _hip.EALIGN), (dict(v=0x10208), _hip.EALIGN),
    (dict(scale=0.0), _hip.EINVAL), (dict(scale=-0.125), _hip.EINVAL), (dict(scale=float("nan")), _hip.EINVAL),
    (dict(q=0), _hip.EINVAL), (dict(k=0), _hip.EINVAL), (dict(v=0), _hip.EINVAL), (dict(kb=0), _hip.EINVAL),
    (dict(km=0), _hip.EINVAL), (dict(kc=0), _hip.EINVAL), (dict(err=0), _hip.EINVAL), (dict(out=0), _hip.EINVAL),
    (dict(lse=0), _hip.EINVAL), (dict(ldo=64), _hip.ESHAPE), (dict(ldo=130), _hip.EALIGN),
]


@pytest.mark.parametrize("kw,code", REFUSALS, ids=[f"{next(iter(k))}={next(iter(k.values()))}" for k, _ in REFUSALS])
def test_refusals_happen_before_any_launch(kw, code):
    lib = _hip.lib()
    assert getattr(lib, FWD)(*_fwd_args(**kw)) == code
    if set(kw) != {"ldo"} or kw["ldo"] != 130:     # (the backward reads `out` in 16-byte pieces: ldo % 8)
        assert getattr(lib, BWD)(*_bwd_args(**kw)) == code


def test_backward_only_refusals_and_empty_batch():
    lib = _hip.lib()
    for name in ("qb", "qm", "qc", "dout", "ws", "dq", "dk", "dv"):
        assert getattr(lib, BWD)(*_bwd_args(**{name: 0})) == _hip.EINVAL, name
    for kw, code in ((dict(lddo=64), _hip.ESHAPE), (dict(ldd=64), _hip.ESHAPE), (dict(ldo=132), _hip.EALIGN),
                     (dict(lddo=132), _hip.EALIGN), (dict(ldd=386), _hip.EALIGN), (dict(dout=0x10008), _hip.EALIGN),
                     (dict(dk=0x10104), _hip.EALIGN)):
        assert getattr(lib, BWD)(*_bwd_args(**kw)) == code, kw
    assert getattr(lib, FWD)(*_fwd_args(B=0)) == _hip.OK
    assert getattr(lib, BWD)(*_bwd_args(B=0)) == _hip.OK
    assert getattr(lib, FWD)(*_fwd_args(B=0, S=100)) == _hip.ESHAPE      # (the checks come first)
