"""The attention parity checks (tests/attention_ref.py) without a GPU: r16 - the float32 computation with the kernels' bf16
rounding points - goes through check_case() in place of a kernel's output, for every case of test_attention_parity_gpu.py.
The bounds are therefore known to be satisfiable by a correctly rounding implementation before a GPU is used; and the same
check refuses small localised errors."""
import pytest
import torch

from tests import attention_ref as ar


@pytest.mark.parametrize("name", list(ar.CASES))
def test_r16_satisfies_every_assertion(name):
    ar.check_case(name, ar.r16_as_kernel_output(name))


def test_cases_cover_what_they_are_meant_to():
    c = ar.CASES
    assert len(c) == 25
    assert any(v["scale"] == 0.2 and v["p"] > 0 and v["mask"] is not None for v in c.values())
    assert c["packed-p0.0"]["lens"] == [1, 33, 63, 64, 65, 0, 127, 129, 256] and c["packed-qlim-p0.25"]["qlim"][-1] == 300
    seqs = ar.sequences(c["packed-qlim-p0.25"])
    assert [s[3] for s in seqs] == [1, 0, 63, 64, 65, 0, 1, 128, 256]
    for name in ("nokey-packed-p0.25", "nokey-pad2x1x1152-p0.1", "nokey-pad2x1x2048-p0.1", "skip4x2x512-p0.1"):
        live = [bool(ar.key_live(c[name], b, lo, n).any()) for b, lo, n, _ in ar.sequences(c[name])]
        assert not all(live) and any(live), name


@pytest.mark.parametrize("name", ["pad2x3x256-mask-p0.1", "packed-qlim-p0.25"])
def test_check_refuses_localised_errors(name):
    """One wrong row, the last row of a ragged sequence, a store past a query limit, one key quad with another dropout
    multiplier in dK only: each must fail."""
    c = ar.CASES[name]
    H = c["NH"] * 64
    r16 = ar.reference(name, "r16")
    cands = [s for s in ar.sequences(c) if s[3] >= 64]
    b, lo, n, nq = ([s for s in cands if s[3] < s[2]] or cands)[-1]     # (one with a query limit, where there is one)
    last_live = int(ar.key_live(c, b, lo, n).nonzero().max())

    def refused(edit):
        got = ar.r16_as_kernel_output(name)
        got = {k: v.clone() for k, v in got.items()}
        edit(got)
        with pytest.raises(AssertionError):
            ar.check_case(name, got)

    def wrong_row(got):          # dQ of one query row of one head: its neighbour's
        got["dqkv"][lo + 5, :64] = got["dqkv"][lo + 6, :64]

    def last_row(got):           # the sequence's last live key never got its dV
        got["dqkv"][lo + last_live, 2 * H:] = 0

    def past_limit(got):         # a store one row past the sequence's query rows (or into the next sequence)
        got["out"][lo + nq, 0] = 0.5

    def dk_quad(got):            # four keys of dK without the 1 / (1-p) of their dropout multiplier
        got["dqkv"][lo + 8:lo + 12, H:H + 64] = (r16["dk"][lo + 8:lo + 12, :64] * (1 - c["p"])).to(torch.bfloat16)

    def lse_guard(got):          # one lse entry that the forward never stores
        got["lse"][b, 0, nq - 1] = float("nan")

    for edit in (wrong_row, last_row, dk_quad, lse_guard) + ((past_limit,) if lo + nq < c["T"] and nq < n else ()):
        refused(edit)
