"""CPU: the step's mask provider (tests/step_dropout_ref.py) and the oracle's dropout hook - what must hold without a GPU,
and the discriminating power of tests/test_step_dropout_gpu.py: ten single mistakes in the engine's dropout bookkeeping,
each restated as a mutant provider, each moving at least one quantity the GPU test compares by 3 x that quantity's GPU
tolerance (fp64 oracle under the mutant's masks against the fp64 oracle under the contract's)."""
import numpy as np
import pytest
import torch

from oracle import stonkgs_oracle as orc
from tests import step_dropout_ref as R
from tests.golden_util import load_case
from tests.test_step_dropout_gpu import ENVELOPE, P, SEED_BASE

STEP = SEED_BASE + 1
FULL = (True, True, True)


@pytest.fixture
def deterministic():
    """The embedding tables' gradients are index-adds, which torch splits among threads in an order of its own: bit-for-bit
    comparisons of two oracle runs need the deterministic kernels."""
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(before)


@pytest.fixture(scope="module")
def case():
    from tests.test_unpad_gpu import _batches

    cfg, sd, tsv_rows, _, _, _ = load_case("g2_hipsmall")
    with torch.no_grad():
        table = orc.build_kg_table(tsv_rows, orc.special_vectors(sd, cfg))
    return dict(cfg=cfg, sd=sd, sd64=R.to64(sd), table=table, batches=_batches(cfg, 4), refs={})


def _correct(case, bi, layout=FULL):
    """(provider, fp64 terms, fp64 gradients, r16) of batch `bi` under the contract's masks - computed once."""
    key = (bi, layout)
    if key not in case["refs"]:
        cfg, batch = case["cfg"], case["batches"][bi]
        prov = R.StepDropout(cfg, batch, STEP, layout, P, P)
        terms, g64 = R.oracle_step(case["sd64"], cfg, case["table"], batch, prov)
        _, g16 = R.oracle_step(case["sd"], cfg, case["table"], batch, prov, autocast=True)
        case["refs"][key] = (prov, terms, g64, {k: R.rel(g16[k], g64[k]) for k in g64})
    return case["refs"][key]


# ------------------------------------------------------------------------------------------ identity
def test_a_provider_with_p_zero_is_the_hook_free_oracle(case, deterministic):
    cfg, batch = case["cfg"], case["batches"][1]
    for sd in (case["sd"], case["sd64"]):
        t0, g0 = R.oracle_step(sd, cfg, case["table"], batch, None)
        t1, g1 = R.oracle_step(sd, cfg, case["table"], batch, R.StepDropout(cfg, batch, STEP, FULL, 0.0, 0.0))
        assert t0 == t1
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k


def test_train_step_takes_the_hook(case, deterministic):
    cfg, batch = case["cfg"], case["batches"][0]
    prov, terms, g64, _ = _correct(case, 0)
    res = orc.train_step({k: v.clone() for k, v in case["sd64"].items()}, cfg, case["table"], batch, orc.AdamState(),
                         max_grad_norm=0.0, dropout=prov)
    assert float(res["loss"]) == terms["loss"]
    for k in g64:
        assert torch.equal(res["grads"][k], g64[k]), k


# ------------------------------------------------------------------------------------------ the masks themselves
def _expected_sigma(n, p):
    return np.sqrt(p * (1 - p) / n)


def test_keep_rates_and_distinct_masks(case):
    """Every site keeps 1 - p of the elements that have a row (5 sigma), no two sites of a step draw the same mask, and
    the scale is 1 / (1 - float32(p))."""
    cfg, batch = case["cfg"], case["batches"][1]
    for layout in R.LAYOUTS:
        prov = R.StepDropout(cfg, batch, STEP, layout, P, P)
        zeroed = R.StepDropout(cfg, batch, STEP, layout, P, P, norow="zeros")
        seen = {}
        for key, shape in prov.sites(classifier=True):
            m = prov.keep(key, shape).numpy()
            assert set(np.unique(m)) <= {0.0, 1.0, R.drop_scale(P)}, key
            # positions without a row are all ones in `prov` and all zeros in `zeroed`: they are left out of the rate
            live = ~((m != 0) & (zeroed.keep(key, shape).numpy() == 0))
            assert (m[~live] == 1.0).all() and set(np.unique(m[live])) <= {0.0, R.drop_scale(P)}, key
            n = int(live.sum())
            rate = float((m[live] != 0).mean())
            assert abs(rate - (1 - P)) < 5 * _expected_sigma(n, P), (layout, key, rate, n)
            seen[key] = (shape, m != 0, live)
        keys = list(seen)
        for a in range(len(keys)):
            for b in range(a + 1, len(keys)):
                (sa, ma, la), (sb, mb, lb) = seen[keys[a]], seen[keys[b]]
                if sa == sb:
                    assert not np.array_equal(ma, mb), (keys[a], keys[b])
                    # ... nor nearly: two independent masks agree on p^2 + (1 - p)^2 = 0.82 of the elements that have a row
                    both = la & lb
                    assert abs(float((ma == mb)[both].mean()) - (P * P + (1 - P) ** 2)) < 0.01, (keys[a], keys[b])


def test_seeds_follow_the_formula(case):
    cfg, batch = case["cfg"], case["batches"][0]
    prov = R.StepDropout(cfg, batch, STEP, FULL, P, P)
    got = {prov.launch(k)[1:3]: prov.seed(*prov.launch(k)[:3]) for k, _ in prov.sites(classifier=True)}
    assert set(got) == {(100, 0), (101, 1), (101, 2), (101, 3), (102, 1), (102, 2), (102, 3), (200, 0), (0, 1), (0, 2), (0, 3),
                        (1, 1), (1, 2), (1, 3), (300, 0)}
    for (layer, site), s in got.items():
        assert s == (STEP * 0x9E3779B1 + layer * 64 + site) % 2 ** 32
    assert len(set(got.values())) == len(got)


def test_packed_and_padded_providers_differ(case):
    cfg, batch = case["cfg"], case["batches"][1]
    padded, packed = (R.StepDropout(cfg, batch, STEP, l, P, P) for l in (R.LAYOUTS[0], R.LAYOUTS[1]))
    pruned, pruned_attn = (R.StepDropout(cfg, batch, STEP, l, P, P) for l in (R.LAYOUTS[2], R.LAYOUTS[3]))
    differs = lambda a, b, key, shape: not np.array_equal(a.keep_bool(key, shape), b.keep_bool(key, shape))   # noqa: E731
    for key, shape in padded.sites():
        if key[0].startswith("lm_backbone."):     # the frozen backbone is padded in every layout
            assert not differs(padded, packed, key, shape) and not differs(padded, pruned_attn, key, shape), key
        else:
            assert differs(padded, packed, key, shape), key
    S, H, NH = cfg.max_position_embeddings, cfg.hidden_size, cfg.num_attention_heads
    l0, l1 = "bert.encoder.layer.0", "bert.encoder.layer.1"
    # the pruned last layer: site 3 moves with prune_last_ffn, site 2 with prune_last_attn, nothing else does
    assert differs(packed, pruned, (l1, 3), (4, S, H)) and not differs(packed, pruned, (l1, 2), (4, S, H))
    assert differs(pruned, pruned_attn, (l1, 2), (4, S, H)) and not differs(pruned, pruned_attn, (l1, 3), (4, S, H))
    for site, shape in ((1, (4, NH, S, S)), (2, (4, S, H)), (3, (4, S, H))):
        assert not differs(packed, pruned_attn, (l0, site), shape)
    assert not differs(packed, pruned_attn, (l1, 1), (4, NH, S, S))
    # sequence 2 of this batch is all live and unlabelled positions follow labelled ones: packed index != position
    assert (packed.local[2 * S:3 * S] != np.arange(S)).any()


def test_positions_without_a_row_are_never_read(case, deterministic):
    """Dropping EVERYTHING at the positions that have no row in the layout (instead of keeping everything there) changes
    no loss term and no gradient, bit for bit: the provider's "all ones" there is a choice without consequence."""
    cfg = case["cfg"]
    for bi, batch in enumerate(case["batches"]):
        for layout in R.LAYOUTS[1:]:
            _, terms, g64, _ = _correct(case, bi, layout)
            flipped = R.StepDropout(cfg, batch, STEP, layout, P, P, norow="zeros")
            n_flipped = sum(int((flipped.keep(k, s) != _correct(case, bi, layout)[0].keep(k, s)).sum()) for k, s in flipped.sites())
            assert n_flipped > 0
            t1, g1 = R.oracle_step(case["sd64"], cfg, case["table"], batch, flipped)
            assert t1 == terms, (bi, layout)
            for k in g64:
                assert torch.equal(g1[k], g64[k]), (bi, layout, k)


# ------------------------------------------------------------------------------------------ discriminating power
MUTANTS = {
    "01a seed of site 1, layer 0": dict(seed_delta={(0, 1): 1}),
    "01b seed of site 2, layer 0": dict(seed_delta={(0, 2): 1}),
    "01c seed of site 3, layer 0": dict(seed_delta={(0, 3): 1}),
    "01d seed of backbone site (100, 0)": dict(seed_delta={(100, 0): 1}),
    "01e seed of backbone site (101, 3)": dict(seed_delta={(101, 3): 1}),
    "02 joint-embedding seed": dict(seed_delta={(200, 0): 1}),
    "03 seed_base + 1": dict(seed_base=STEP + 1),
    "04 padded rows in the packed layout": dict(rows="padded"),
    "05 packed row for the read row, site 3": dict(read_rows=(3,)),
    "06 packed row for the read row, site 2": dict(read_rows=(2,)),
    "07 attention keyed by position": dict(attn_index="position"),
    "08 backward mask != forward mask, site 2": dict(backward_seed_delta={(0, 2): 1}),
    "09 backward mask != forward mask, attention": dict(backward_seed_delta={(0, 1): 1}),
    "10 backbone drawn with the previous counter": dict(backbone_base=STEP - 1),
}


def mutant_distances(case, bi, kw, layout=FULL):
    """[(quantity, distance, GPU tolerance)] of the mutant `kw` from the contract on batch `bi`."""
    kw = dict(kw)
    cfg, batch = case["cfg"], case["batches"][bi]
    _, terms, g64, r16 = _correct(case, bi, layout)
    mutant = R.StepDropout(cfg, batch, kw.pop("seed_base", STEP), layout, P, P, **kw)
    m_terms, m64 = R.oracle_step(case["sd64"], cfg, case["table"], batch, mutant)
    rows = [(k, abs(m_terms[k] - terms[k]), R.LOSS_ATOL) for k in R.TERMS]
    for k, g in g64.items():
        if float(g.norm()) < 1e-5:
            rows.append((k, R.rel(m64[k], g), R.ZERO_REF_TOL))
        else:
            rows.append((k, R.rel(m64[k], g), ENVELOPE["max"] * r16[k]))
    return rows


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_is_caught_at_three_times_the_gpu_tolerance(case, name):
    """In the default layout (packed, last layer pruned, attention too): among the quantities the GPU test compares - four
    loss terms and every gradient tensor, on each of the two batches - at least one moves by >= 3 x its GPU tolerance (loss
    terms: 1e-2; a gradient tensor: ENVELOPE["max"] x its r16). Every mutant but 01e is caught on BOTH batches; a seed slip at
    a site INSIDE a frozen-backbone layer moves the trainable step least (profiles/step_dropout_parity.md)."""
    best = []
    for bi in range(2):
        rows = mutant_distances(case, bi, MUTANTS[name])
        k, d, tol = max(rows, key=lambda r: r[1] / r[2])
        caught = sum(1 for r in rows if r[1] >= 3 * r[2])
        print(f"{name}, batch {bi}: worst {k} distance {d:.3e} = {d / tol:.1f} x tolerance {tol:.3e}; {caught} of {len(rows)} "
              "quantities at >= 3 x")
        best.append(d / tol)
    assert max(best) >= 3, (name, best)
    if not name.startswith("01e"):
        assert min(best) >= 3, (name, best)
