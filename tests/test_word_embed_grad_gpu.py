"""GPU: stonk_word_embed_grad (csrc/text_embed.hip) - the gradient of a trainable word-embedding lookup - against an fp64
index_add_, with a hot destination row, the padding row, the packed layout, row strides wider than H, a preset table
(accumulation) and guard rows around it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 3, 256
HOT, N_HOT = 7, 220


def _case(H, vocab, packed, seed=0):
    g = torch.Generator().manual_seed(seed + H + vocab)
    n = B * S
    ids = torch.randint(1, vocab - 1, (n,), generator=g)
    where = torch.randperm(n, generator=g)
    ids[where[:N_HOT]] = HOT                       # one destination row with far more adders than a wavefront has lanes
    ids[where[N_HOT:N_HOT + 12]] = 0               # the padding id at live positions
    ids[where[N_HOT + 12:N_HOT + 17]] = vocab - 1  # the last row of the table
    row_of_pos = None
    if packed:   # a permutation of the rows with about a third of the positions dropped
        row_of_pos = torch.randperm(n, generator=g).to(torch.int32)
        row_of_pos[torch.randperm(n, generator=g)[:n // 3]] = -1
    ld, ld_w = H + 8, H + 5
    dsum = torch.zeros(n, ld, dtype=torch.bfloat16)
    dsum[:, :H] = torch.randn(n, H, generator=g).to(torch.bfloat16)
    dsum[:, H:] = 1000.0                           # never read: would show in every sum
    table = torch.randn(vocab + 2, ld_w, generator=g)   # rows 0 and vocab + 1: guards
    return ids.view(B, S), row_of_pos, dsum, table, ld, ld_w


def _run(hip, ids, row_of_pos, dsum, table, ld, ld_w, H, vocab, padding_idx, batch=B):
    """Returns (table after the call, error word)."""
    dev = "cuda"
    ids_d, dsum_d, tab_d = ids.to(dev).contiguous(), dsum.to(dev), table.clone().to(dev)
    rop_d = None if row_of_pos is None else row_of_pos.to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.call("stonk_word_embed_grad", dsum_d.data_ptr(), ld, ids_d.data_ptr(), hip.ptr(rop_d), tab_d[1].data_ptr(), ld_w,
             vocab, padding_idx, batch, S, H, err.data_ptr(), hip.stream_ptr())
    torch.cuda.synchronize()
    return tab_d.cpu(), int(err.item())


def _reference(ids, row_of_pos, dsum, table, H, vocab, padding_idx):
    """fp64 sums, the sums of absolute values and the number of contributions per destination row."""
    flat = ids.reshape(-1)
    rows = torch.arange(flat.numel()) if row_of_pos is None else row_of_pos.long()
    live = (rows >= 0) & (flat != padding_idx)
    contrib = dsum[rows[live], :H].double()
    ref = table[1:vocab + 1, :H].double().clone()
    mag = ref.abs()
    ref.index_add_(0, flat[live], contrib)
    mag.index_add_(0, flat[live], contrib.abs())
    count = torch.bincount(flat[live], minlength=vocab)
    return ref, mag, count


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("H,vocab", [(128, 160), (128, 1000), (768, 160), (768, 1000)])
def test_word_embed_grad_against_fp64_index_add(hip, H, vocab, packed):
    ids, row_of_pos, dsum, table, ld, ld_w = _case(H, vocab, packed)
    for padding_idx in (0, -1):
        got, err = _run(hip, ids, row_of_pos, dsum, table, ld, ld_w, H, vocab, padding_idx)
        ref, mag, count = _reference(ids, row_of_pos, dsum, table, H, vocab, padding_idx)
        assert err == 0
        assert count[HOT] >= (N_HOT * 0.55 if packed else N_HOT) and count[vocab - 1] >= 1
        body = got[1:vocab + 1, :H]
        # fp32 running sum of n contributions onto the preset: n additions, each within 2^-24 of a partial sum that |preset| +
        # sum |contribution| bounds, in any arrival order; a factor of two on top
        bound = count[:, None].double() * 2.0 ** -23 * mag
        excess = ((body.double() - ref).abs() - bound).max()
        print(f"H={H} vocab={vocab} packed={packed} pad={padding_idx}: max |got - ref| = "
              f"{(body.double() - ref).abs().max():.3e}, hot row n = {int(count[HOT])}, worst excess over the bound = {excess:.3e}")
        assert excess <= 0
        untouched = count == 0
        assert torch.equal(body[untouched], table[1:vocab + 1, :H][untouched])           # bit-identical
        assert torch.equal(got[:, H:], table[:, H:])                                     # the columns past H
        assert torch.equal(got[0], table[0]) and torch.equal(got[vocab + 1], table[vocab + 1])   # the guard rows
        if padding_idx == 0:
            assert untouched[0] and (ids == 0).sum() >= 12
        else:
            assert count[0] >= 1 and not torch.equal(body[0], table[1, :H])              # row 0 receives its sum


def test_out_of_range_ids_raise_the_flag_and_touch_nothing(hip):
    H, vocab = 128, 160
    ids, row_of_pos, dsum, table, ld, ld_w = _case(H, vocab, True)
    bad = torch.tensor([-1, vocab, -(1 << 40), vocab + 5, 1 << 40, -3])
    ids = bad[torch.arange(B * S) % bad.numel()].view(B, S)
    got, err = _run(hip, ids, row_of_pos, dsum, table, ld, ld_w, H, vocab, 0)
    assert err & 1 and torch.equal(got, table)
    # one id below 0 and one >= vocab among valid ones: the others are summed as if the two were not there
    ids, row_of_pos, dsum, table, ld, ld_w = _case(H, vocab, False)
    ids[0, 3], ids[2, 250] = -3, vocab
    got, err = _run(hip, ids, row_of_pos, dsum, table, ld, ld_w, H, vocab, 0)
    keep = torch.ones(B * S, dtype=torch.int32)
    keep[3], keep[2 * S + 250] = -1, -1
    ref, mag, count = _reference(ids.clamp(0, vocab - 1), torch.where(keep > 0, torch.arange(B * S, dtype=torch.int32), keep),
                                 dsum, table, H, vocab, 0)
    assert err & 1
    assert ((got[1:vocab + 1, :H].double() - ref).abs() <= count[:, None].double() * 2.0 ** -23 * mag).all()
    assert torch.equal(got[0], table[0]) and torch.equal(got[vocab + 1], table[vocab + 1]) and torch.equal(got[:, H:], table[:, H:])


def test_empty_batch_leaves_everything_untouched(hip):
    H, vocab = 128, 160
    ids, row_of_pos, dsum, table, ld, ld_w = _case(H, vocab, False)
    got, err = _run(hip, ids, row_of_pos, dsum, table, ld, ld_w, H, vocab, 0, batch=0)
    assert err == 0 and torch.equal(got, table)
