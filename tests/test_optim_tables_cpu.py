"""CPU (no GPU): the span tables the optimizer kernels are driven with, in integers. The decay table of FusedAdamW and the
pieces a sharded optimizer owns (GradSynchronizer.owned_spans on plan_buckets' output, world sizes 2 and 8) for the flat
layout of a real two-layer model; and check_tables - the contract of stonk_adamw_step_tiled as test_optim_parity_gpu.py
asserts it for Engine.adamw_tables() - refuses a hole, an overlap and a misaligned entry."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests import optim_ref as orf


def _store():
    from stonkgs_amd.config import STonKGsConfig
    from stonkgs_amd.params import FlatStore, trainable_specs

    cfg = STonKGsConfig(vocab_size=1000, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                        intermediate_size=256, max_position_embeddings=256)
    return cfg, FlatStore(trainable_specs(cfg), "cpu", True)


def test_decay_table_is_the_stored_extent_of_every_weight_that_is_no_layernorm():
    from stonkgs_amd.stonkgs_pretraining import FusedAdamW

    cfg, store = _store()
    opt = FusedAdamW(store, weight_decay=0.01)
    spans = [tuple(r) for r in opt._decay_table().tolist()]
    want = sorted((off, off + math.prod(pshape)) for name, (off, _, pshape) in store.index.items()
                  if name.endswith(".weight") and "LayerNorm" not in name)
    assert spans == want and len(spans) == 4 * cfg.num_hidden_layers + 7
    orf.check_spans(spans, store.numel)
    # every tensor is decayed wholly or not at all, and the alignment gap behind a decayed tensor is not
    mask = orf.span_mask(store.numel, spans)
    for name, (off, _, pshape) in store.index.items():
        n, end = math.prod(pshape), store.span(name)[1]
        assert bool(mask[off:off + n].all()) == (name.endswith(".weight") and "LayerNorm" not in name), name
        assert not mask[off:off + n].any() or mask[off:off + n].all()
        assert not mask[off + n:end].any(), name
    assert opt._pieces() == [(0, 0, store.numel)]


@pytest.mark.parametrize("world", [2, 8])
def test_owned_spans_cut_every_bucket_into_aligned_pieces_that_cover_the_buffer_once(world):
    from stonkgs_amd.stonkgs_pretraining import FusedAdamW, GradSynchronizer, plan_buckets, segment_ends_for

    cfg, store = _store()
    seg = segment_ends_for(SimpleNamespace(_store=store, config=cfg))
    mb = 0.25
    buckets = plan_buckets(sorted(set(seg.values())), int(mb * (1 << 20) / 4))
    assert len(buckets) >= 3 and buckets[0][0] == 0 and buckets[-1][1] == store.numel
    assert all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
    count = torch.zeros(store.numel, dtype=torch.int32)
    for rank in range(world):
        sync = GradSynchronizer(store.grad, seg, bucket_mb=mb, shard=True, comm=SimpleNamespace(world=world, rank=rank))
        assert sync.shard and sync.buckets == buckets
        spans = sync.owned_spans()
        assert len(spans) == len(buckets)
        for (lo, hi), (blo, bhi) in zip(spans, buckets):
            piece = (bhi - blo) // world
            assert piece * world == bhi - blo and (lo, hi) == (blo + rank * piece, blo + (rank + 1) * piece)
            assert lo % 4 == 0 and hi % 4 == 0        # 16-byte aligned fp32, 8-byte aligned bf16: what stonk_adamw_step needs
            count[lo:hi] += 1
        orf.check_spans(spans, store.numel)
        # the optimizer's pieces: span_base = the piece's own offset, m / v packed behind each other
        opt = FusedAdamW(store, spans=spans)
        pieces, acc = opt._pieces(), 0
        assert [(off, n) for off, _, n in pieces] == [(lo, hi - lo) for lo, hi in spans]
        for off, soff, n in pieces:
            assert soff == acc and soff % 4 == 0 and n % 4 == 0
            acc += n
        assert acc == opt.m.numel() == opt.v.numel() == store.numel // world
    assert (count == 1).all()
    # pieces begin inside tensors, not only at their boundaries - what span_base is for
    starts = {off for off, _, _ in store.index.values()}
    assert any(lo not in starts for lo, _ in spans)


def test_check_tables_accepts_the_layout_and_refuses_a_hole_an_overlap_and_a_misalignment():
    index, numel = orf.layout()
    tiles, n_tiles, spans, chunks = orf.host_tables(index, numel, lambda name: 4096)
    ext = orf.check_tables(numel, tiles, n_tiles, spans, chunks)
    assert [k for _, _, k in ext].count("tile") == 4 and ext[-1][1] == numel
    assert orf.unpack_tiles(orf.pack_tiles(tiles)) == tiles
    # every tensor lies wholly in one table
    for name, (off, _, _, n) in index.items():
        assert sum(lo <= off and off + n <= hi for lo, hi, _ in ext) == 1, name

    def refused(tiles=tiles, n_tiles=n_tiles, spans=spans, chunks=chunks, numel=numel):
        with pytest.raises(AssertionError):
            orf.check_tables(numel, tiles, n_tiles, spans, chunks)

    refused(spans=spans[:1] + spans[2:])                                            # a hole: those tensors would stop training
    refused(spans=[(spans[0][0] - 4,) + spans[0][1:]] + spans[1:])                    # four elements updated twice
    refused(spans=[spans[0][:2] + (1,)] + spans[1:])                                  # first_chunk off by one
    refused(chunks=chunks + 1)
    refused(n_tiles=n_tiles - 1)
    refused(tiles=[tiles[0][:1] + (4104,) + tiles[0][2:]] + tiles[1:])                # a W^T copy that is not 16-byte aligned
    refused(tiles=[tiles[0][:2] + (128,) + tiles[0][3:]] + tiles[1:])                 # ld_out below roundup64(rows)
    refused(tiles=[tiles[0][:4] + (tiles[0][4] - 64,) + tiles[0][5:]] + tiles[1:])    # pad rows in neither table
    refused(numel=numel + 4)
