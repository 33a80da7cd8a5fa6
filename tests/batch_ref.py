"""Case tables, input builders, checks and launch constants of the three integer kernels every training step runs before
its first GEMM, for tests/test_batch_parity_gpu.py: csrc/unpad.hip (stonk_unpad_plan - which rows the trainable encoder
runs on, in which order) and csrc/data.hip (stonk_mlm_mask, stonk_assemble_rows - the batch itself).
tests/test_batch_ref_cpu.py pins all of it without a GPU. CPU only: nothing here touches a device.

Every case is there for one branch of a kernel, named where the case is built. Whether the branch is taken depends on
constants of the launchers (256 threads per sequence, the 64-thread block of the masking kernel, its 8192-key LDS limit,
the 256-thread block of the assembly kernel); `geometry()` reads those out of the launchers' own source lines, so that a
launcher edited without its case fails the CPU file by name.

THE RULE: integer work, no tolerance anywhere. A kernel's outputs must EQUAL the restatement (oracle/masking_oracle.py)
and, separately, satisfy invariants computed from the outputs and the inputs alone (`plan_invariants`, `mask_invariants`,
`assemble_invariants`), which do not go through the restatement: a mistake the kernel and the restatement share still fails.
The `*_model` functions restate the kernels a SECOND time, shaped like the kernels (threads, chunks, scans, rank by
counting), with ONE MISTAKE each on request (`wrong=`): the CPU file shows that the model without a mistake equals the
restatement on every case and that every mistake is told apart by a named case."""
import functools
import os
import re

import numpy as np

from oracle import masking_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stonkgs_amd", "csrc")
M = 0xFFFFFFFF
UNWRITTEN = -7            # what the models leave in an element no thread writes


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry, from the launchers' source
# ---------------------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the launcher's line is not what tests/batch_ref.py reads - re-read it and re-size the case"
    return m


@functools.lru_cache(maxsize=None)
def geometry():
    """The constants the cases are sized by: {name: int}."""
    g = {}
    up, da = _src("unpad.hip"), _src("data.hip")
    g["tpb"] = int(_find(r"constexpr int TPB = (\d+);", up, "unpad TPB").group(1))
    _find(r"const int per = \(S \+ TPB - 1\) / TPB;", up, "unpad chunk size")
    _find(r"const int s0 = threadIdx\.x \* per, s1 = s0 \+ per < S \? s0 \+ per : S;", up, "unpad chunk bounds")
    _find(r"for \(int s = threadIdx\.x; s < S; s \+= TPB\) live \|= ", up, "unpad live scan")
    _find(r"for \(int j = threadIdx\.x; j < B; j \+= TPB\) \{", up, "unpad count loop")
    _find(r"for \(long i = all \+ \(long\)b \* TPB \+ threadIdx\.x; i < cap; i \+= \(long\)B \* TPB\)", up, "unpad tail fill")
    for k in ("unpad_count_kernel", "unpad_fill_kernel"):
        _find(rf"hipLaunchKernelGGL\({k}, dim3\(B\), dim3\(TPB\), 0, st,", up, k + " launch")
    g["ws_per_seq"] = int(_find(r"return B > 0 \? (\d+)L \* B : 0;", up, "unpad workspace").group(1))
    _find(r"ws_ints >= 3L \* B", up, "unpad workspace check")
    g["mask_block"] = int(_find(r"__launch_bounds__\((\d+)\) void mlm_mask_kernel", da, "mask block").group(1))
    m = _find(r"hipLaunchKernelGGL\(mlm_mask_kernel, dim3\(2 \* B\), dim3\((\d+)\), half \* sizeof\(uint32_t\),", da, "mask launch")
    assert int(m.group(1)) == g["mask_block"], "mask launch"
    _find(r"for \(int pos = lane; pos < half; pos \+= (\d+)\)", da, "mask position loop")
    g["mask_half_limit"] = int(_find(r"S == 2 \* half && half <= (\d+),", da, "mask LDS limit").group(1))
    m = _find(r"hipLaunchKernelGGL\(assemble_kernel, dim3\(\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\),", da,
              "assemble launch")
    assert int(m.group(1)) + 1 == int(m.group(2)) == int(m.group(3)), "assemble launch"
    g["assemble_block"] = int(m.group(3))
    return g


# ---------------------------------------------------------------------------------------------------------------------
# the counter-based stream on Python ints, and its inverse
# ---------------------------------------------------------------------------------------------------------------------
def h32(x):
    """lowbias32 (stonk_hash32) on a Python int."""
    x &= M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def unh32(y):
    """The inverse of h32: every step of lowbias32 is a bijection of 32-bit words."""
    y ^= y >> 16
    y = (y * pow(0x846CA68B, -1, 1 << 32)) & M
    y ^= (y >> 15) ^ (y >> 30)
    y = (y * pow(0x7FEB352D, -1, 1 << 32)) & M
    y ^= y >> 16
    return y


def base_key(seed):
    return h32((seed * mo.K_SEED + mo.K_SEED_ADD) & M)


def neg_draw(seed, b):
    """The word row b compares with the negative threshold."""
    return h32(base_key(seed) ^ ((b * mo.K_NEG) & M))


def partner_draw(seed, b, B):
    """The partner row b draws BEFORE the fallback."""
    return (h32(base_key(seed) ^ ((b * mo.K_PART) & M)) * B) >> 32


def seed_for_neg_draw(value, b):
    """The seed for which row b draws `value`: the seed mix and lowbias32 run backwards."""
    base = unh32(value) ^ ((b * mo.K_NEG) & M)
    return ((unh32(base) - mo.K_SEED_ADD) * pow(mo.K_SEED, -1, 1 << 32)) & M


def thr_float(rate):
    """stonk_drop_thr32 of the ABI's float argument."""
    return mo.drop_thr32(rate)


def thr_double(rate):
    """THE OLD RULE of the restatement: the threshold from the Python double."""
    return int(rate * 4294967296.0 + 0.5)


def gap_seed(rate, b=1):
    """(seed, draw, lo, hi): a seed whose row b draws the middle of the gap [lo, hi) between the two thresholds."""
    lo, hi = sorted((thr_float(rate), thr_double(rate)))
    draw = (lo + hi) // 2
    return seed_for_neg_draw(draw, b), draw, lo, hi


# ---------------------------------------------------------------------------------------------------------------------
# row plan: cases
# ---------------------------------------------------------------------------------------------------------------------
MASK_WORDS = (1, 2, -1, 1 << 40)


def _plan_random(B, S, half, seed, text=True, ent=True):
    """Prefix masks of random length with holes, live words from MASK_WORDS, labels on 15 % of both halves - among them a
    label AT position 0 (tl[0, 0]: counted once), the value -1 (tl[0, half - 1]) and 1 << 40 (el[B - 1, 0])."""
    rng = np.random.RandomState(seed)
    am = np.zeros((B, S), dtype=np.int64)
    for b in range(B):
        n = rng.randint(1, S + 1)
        am[b, :n] = rng.choice(MASK_WORDS, n)
        am[b, rng.rand(S) < 0.1] = 0
    labels = []
    for use in (text, ent):
        lab = np.full((B, half), -100, dtype=np.int64)
        pick = rng.rand(B, half) < 0.15
        lab[pick] = rng.randint(0, 1000, int(pick.sum()))
        labels.append(lab if use and half > 0 else None)
    tl, el = labels
    if tl is not None:
        tl[0, 0], tl[0, half - 1] = 7, -1
    if el is not None:
        el[B - 1, 0] = 1 << 40
    return dict(am=am, tl=tl, el=el, half=half)


@functools.lru_cache(maxsize=None)
def plan_cases():
    """name -> dict(am [B, S], tl / el [B, half] or None, half). The branch a case owns:
      s6, s64        fewer positions than threads: chunk 1, most threads hold nothing
      s255           one thread short of a full block, odd S (half = 127: position 254 = 2 half has no label)
      s257           chunk 2: thread 128 holds position 256 alone, threads 129 .. 255 nothing; odd S
      s1000          chunk 4: threads from 250 on start at or beyond S
      s4096          BigBird's length: chunk 16, every thread busy
      b1, b257, b600 the 256-entry count loop: one sequence; a second trip for thread 0; a third trip
      half0_null     the text baseline's call: half = 0, no label pointers
      half0_ent      half = 0 with a non-null entity pointer (all words labelled): never read
      half_S         half = S: every position a text position, the entity pointer (all labelled) never read
      s260_h256      entity labels exist for 4 positions only (s - half < half holds, s < S ends it)
      s512_h100      positions >= 200 are kept by their mask word alone; el[1, 0] is labelled and am[0, 200] = 0: an
                     entity test `s - half <= half` reads it for position 200 of sequence 0
      text_only, ent_only, neither     label pointers
      last_key       S = 500: the only live key is position 499 (second trip of the live scan, thread 243: the last wave)
      first_key      the only live key is position 0
      all_dead       no sequence has a live key: everything kept, the total is B S
      all_live       every key live: the total is B S, the tail fills take no trip
      tail_fill      B 3, S 4096, one row kept per sequence: the tail fill takes 16 grid-stride trips
      dead_labels    a dead sequence between two others carries labels: its read rows come first, all S are kept"""
    c = {}
    c["s6"] = _plan_random(3, 6, 3, 1)
    c["s64"] = _plan_random(2, 64, 32, 2)
    c["s255"] = _plan_random(2, 255, 127, 3)
    c["s257"] = _plan_random(2, 257, 128, 4)
    c["s257"]["am"][:, 255:] = 2                                        # (the last chunk's positions are live)
    c["s1000"] = _plan_random(2, 1000, 500, 5)
    c["s4096"] = _plan_random(2, 4096, 2048, 6)
    c["b1"] = _plan_random(1, 64, 32, 7)
    c["b257"] = _plan_random(257, 6, 3, 8)
    c["b600"] = _plan_random(600, 10, 5, 9)
    c["half0_null"] = _plan_random(3, 128, 0, 10)
    c["half0_ent"] = _plan_random(3, 128, 0, 11)
    c["half0_ent"]["el"] = np.full((3, 8), 3, dtype=np.int64)
    c["half_S"] = _plan_random(2, 64, 64, 12)
    c["half_S"]["el"] = np.full((2, 64), 3, dtype=np.int64)
    c["s260_h256"] = _plan_random(2, 260, 256, 13)
    c["s260_h256"]["am"][:, 200:] = 0
    c["s260_h256"]["el"][0, [1, 3, 4, 200]] = 9                         # (1 and 3 have positions 257, 259; 4 and 200 none)
    c["s512_h100"] = _plan_random(2, 512, 100, 14)
    c["s512_h100"]["am"][0, 150:] = 0
    c["s512_h100"]["am"][0, 300] = 2
    c["s512_h100"]["el"][1, 0] = 9
    c["text_only"] = _plan_random(3, 64, 32, 15, ent=False)
    c["ent_only"] = _plan_random(3, 64, 32, 16, text=False)
    c["neither"] = _plan_random(3, 64, 32, 17, text=False, ent=False)
    for name, seed in (("last_key", 18), ("first_key", 19), ("all_dead", 20), ("all_live", 21)):
        S = 500 if name == "last_key" else 300
        c[name] = _plan_random(2, S, S // 2, seed)
        c[name]["am"][:] = 1 if name == "all_live" else 0
    c["last_key"]["am"][:, 499] = 1 << 40
    c["first_key"]["am"][:, 0] = -1
    c["tail_fill"] = _plan_random(3, 4096, 2048, 22, text=False, ent=False)
    c["tail_fill"]["am"][:] = 0
    c["tail_fill"]["am"][:, 0] = 1
    c["dead_labels"] = _plan_random(3, 64, 32, 23)
    c["dead_labels"]["am"][1] = 0
    c["dead_labels"]["tl"][1, [3, 9]] = 4
    c["dead_labels"]["el"][1, 5] = 4
    for case in c.values():
        case["am"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def plan_expected(name):
    """The restatement's seven arrays for a case, computed once."""
    c = plan_cases()[name]
    out = mo.unpad_plan(c["am"], c["tl"], c["el"], read=True, half=c["half"])
    for a in out:
        a.setflags(write=False)
    return out


PLAN_NAMES = ("row_of_pos", "pos_of_row", "seq_offsets", "row_mask", "read_rows", "read_of_pos", "read_offsets")


def plan_rule(c):
    """(kept [B, S], read [B, S]) by the rule of unpad.hip's header comment, evaluated position by position."""
    am, tl, el, half = c["am"], c["tl"], c["el"], c["half"]
    B, S = am.shape
    s = np.arange(S)
    lab = np.zeros((B, S), dtype=bool)
    if tl is not None and half > 0:
        t = s[s < half]
        lab[:, t] = np.asarray(tl).reshape(B, half)[:, t] != -100
    if el is not None and half > 0:
        e = s[(s >= half) & (s < 2 * half)]
        lab[:, e] = np.asarray(el).reshape(B, half)[:, e - half] != -100
    read = lab | (s == 0)[None]
    dead = ~(am != 0).any(axis=1)
    return (am != 0) | read | dead[:, None], read


def plan_invariants(c, outs, read=True):
    """What must hold of the kernel's outputs, from them and the inputs alone. outs: the seven arrays (the last three are
    ignored with read=False)."""
    am = c["am"]
    B, S = am.shape
    n = B * S
    rop, por, cu, rm = (np.asarray(a) for a in outs[:4])
    kept, rd = plan_rule(c)
    kept_f, rd_f = kept.reshape(-1), rd.reshape(-1)
    assert rop.shape == (n,) and por.shape == (n,) and cu.shape == (B + 1,) and rm.shape == (n,)
    assert np.array_equal(rop >= 0, kept_f), "the kept set is not the header comment's rule"
    assert (rop[~kept_f] == -1).all()
    total = int(kept.sum())
    assert cu[0] == 0 and np.array_equal(np.diff(cu), kept.sum(axis=1)) and cu[B] == total
    p = np.flatnonzero(kept_f)
    assert (rop[p] < total).all() and np.array_equal(por[rop[p]], p), "pos_of_row does not invert row_of_pos"
    assert (por[total:] == -1).all() and (rm[total:] == 0).all(), "rows past the total"
    assert np.array_equal(rm[:total], am.reshape(-1)[por[:total]]), "row_mask is not the raw mask word of its position"
    for b in range(B):
        rows = por[cu[b]:cu[b + 1]]
        assert ((rows >= b * S) & (rows < (b + 1) * S)).all(), "a sequence's rows are not its own interval"
        flags = rd_f[rows]
        k = int(flags.sum())
        assert flags[:k].all(), "read rows are not a prefix"
        assert (np.diff(rows[:k]) > 0).all() and (np.diff(rows[k:]) > 0).all(), "position order"
    if not read:
        return total
    rr, rofp, ro = (np.asarray(a) for a in outs[4:])
    n_rd = int(rd.sum())
    assert ro[0] == 0 and np.array_equal(np.diff(ro), rd.sum(axis=1)) and ro[B] == n_rd
    assert (rr[n_rd:] == -1).all(), "read rows past their count"
    assert np.array_equal(rofp >= 0, rd_f) and (rofp[~rd_f] == -1).all()
    q = np.flatnonzero(rd_f)
    assert np.array_equal(rr[rofp[q]], rop[q]), "read_of_pos does not index read_rows"
    for b in range(B):
        assert np.array_equal(rr[ro[b]:ro[b + 1]], cu[b] + np.arange(ro[b + 1] - ro[b])), "read rows are not the first rows"
    assert np.array_equal(por[rr[ro[:-1]]], np.arange(B) * S), "a sequence's first read row is not its position 0"
    return total


def plan_facts(name):
    """What the launch of a case does, from its shape and the launch constants."""
    c = plan_cases()[name]
    tpb = geometry()["tpb"]
    B, S = c["am"].shape
    per = -(-S // tpb)
    s0 = np.arange(tpb) * per
    held = np.clip(np.minimum(s0 + per, S) - s0, 0, None)
    total = int(plan_rule(c)[0].sum())
    return dict(per=per, idle=int((held == 0).sum()), beyond=int((s0 > S).sum()), last_held=int(held[held > 0][-1]),
                last_thread=int(np.flatnonzero(held)[-1]), live_trips=-(-S // tpb), count_trips=-(-B // tpb),
                total=total, tail_trips=-(-(B * S - total) // (B * tpb)))


PLAN_WRONG = ("ent_le", "read_not_first", "live_first_block", "floor_chunk", "prefix_le")


def plan_model(c, wrong=None):
    """unpad.hip thread by thread: the live scan, the chunk of every thread, the two exclusive scans, the count loop, the
    tail fills. Elements no thread writes hold UNWRITTEN. wrong:
      "ent_le"            the entity test is `s - half <= half` (one label word too many, the next row's first)
      "read_not_first"    a sequence's rows in plain position order
      "live_first_block"  liveness from the first trip of the live scan only (the first 256 positions)
      "floor_chunk"       the chunk size rounds down
      "prefix_le"         the count loop's prefix is `j <= b`"""
    tpb = geometry()["tpb"]
    am, half = c["am"], c["half"]
    B, S = am.shape
    n = B * S
    tl = None if c["tl"] is None else np.asarray(c["tl"]).reshape(-1)
    el = None if c["el"] is None else np.asarray(c["el"]).reshape(-1)

    def labelled(flat, i):
        return flat is not None and 0 <= i < len(flat) and flat[i] != -100

    def is_read(b, s):
        if s == 0:
            return True
        if s < half:
            return labelled(tl, b * half + s)
        inside = s - half <= half if wrong == "ent_le" else s - half < half
        return inside and labelled(el, b * half + (s - half))

    live = [(am[b, :tpb] if wrong == "live_first_block" else am[b]).any() for b in range(B)]
    rdm = np.array([[is_read(b, s) for s in range(S)] for b in range(B)])
    keepm = rdm | (am != 0) | ~np.array(live)[:, None]
    counts, rcounts = keepm.sum(axis=1), rdm.sum(axis=1)
    out = [np.full(n, UNWRITTEN, dtype=np.int32), np.full(n, UNWRITTEN, dtype=np.int32),
           np.full(B + 1, UNWRITTEN, dtype=np.int32), np.full(n, UNWRITTEN, dtype=np.int64),
           np.full(n, UNWRITTEN, dtype=np.int32), np.full(n, UNWRITTEN, dtype=np.int32),
           np.full(B + 1, UNWRITTEN, dtype=np.int32)]
    rop, por, cu, rm, rr, rofp, ro = out
    per = S // tpb if wrong == "floor_chunk" else -(-S // tpb)
    all_, rall = int(counts.sum()), int(rcounts.sum())
    for b in range(B):
        upto = b + 1 if wrong == "prefix_le" else b
        before, rbefore = int(counts[:upto].sum()), int(rcounts[:upto].sum())
        chunks = [(t * per, min(t * per + per, S)) for t in range(tpb)]
        cnt_r = [int(rdm[b, a:z].sum()) if z > a else 0 for a, z in chunks]
        cnt_o = [int((keepm[b, a:z] & ~rdm[b, a:z]).sum()) if z > a else 0 for a, z in chunks]
        if wrong == "read_not_first":
            cnt_o = [r + o for r, o in zip(cnt_r, cnt_o)]
            scan_r = np.concatenate([[0], np.cumsum(cnt_o)[:-1]])
            scan_o, n_read_b = scan_r, 0
        else:
            scan_r = np.concatenate([[0], np.cumsum(cnt_r)[:-1]])
            scan_o = np.concatenate([[0], np.cumsum(cnt_o)[:-1]])
            n_read_b = sum(cnt_r)
        seen_read = 0
        for t, (a, z) in enumerate(chunks):
            row_r, row_o = before + int(scan_r[t]), before + n_read_b + int(scan_o[t])
            for s in range(a, z):
                p = b * S + s
                r, k = bool(rdm[b, s]), bool(keepm[b, s])
                if wrong == "read_not_first":
                    row = -1
                    if k:
                        row, row_o = row_o, row_o + 1
                    ri = rbefore + seen_read if r else -1
                    seen_read += r
                else:
                    row = -1
                    if r:
                        row, row_r = row_r, row_r + 1
                    elif k:
                        row, row_o = row_o, row_o + 1
                    ri = rbefore + (row - before) if r else -1
                rop[p] = row
                if k and 0 <= row < n:
                    por[row], rm[row] = p, am[b, s]
                rofp[p] = ri
                if r and 0 <= ri < n:
                    rr[ri] = row
        cu[b], ro[b] = before, rbefore
    cu[B], ro[B] = all_, rall
    por[all_:], rm[all_:], rr[rall:] = -1, 0, -1
    return out


def same_plan(a, b, read=True):
    return all(np.array_equal(x, y) for x, y in list(zip(a, b))[:7 if read else 4])


# ---------------------------------------------------------------------------------------------------------------------
# masking: cases
# ---------------------------------------------------------------------------------------------------------------------
def _mask_case(B, half, k_text, k_ent, vocab_text, vocab_ent, mask_id, seed, big_ids=False):
    rng = np.random.RandomState(half * 7 + B)
    ids = rng.randint(1000, 30000, (B, 2 * half)).astype(np.int64)
    if big_ids:
        ids += (1 << 32) + (np.arange(2 * half, dtype=np.int64) << 33)[None]
    ids.setflags(write=False)
    return dict(ids=ids, half=half, k_text=k_text, k_ent=k_ent, vocab_text=vocab_text, vocab_ent=vocab_ent, mask_id=mask_id,
                seed=seed)


@functools.lru_cache(maxsize=None)
def mask_cases():
    """name -> dict(ids [B, 2 half], half, k_text, k_ent, vocab_text, vocab_ent, mask_id, seed). What each owns:
      h1          one key per half: k = half (text) and k = 0 (entity); seed 0
      h2_b1000    2000 workgroups of two keys, k_text != k_ent
      h63, h65    one position short of / beyond the 64 lanes: a partial trip, a second trip of one lane; k = 0, k = half,
                  vocabulary 1 (every random id is 0) and 2^32 - 1 (ids above 2^31: compared as int64), a negative mask id
      h100        k_text != k_ent, input ids above 2^32, a mask id above 2^31, seed 0xFFFFFFFF
      h8192       the LDS limit: 32 KiB of keys, 128 trips per lane, k = half in the entity half"""
    limit = geometry()["mask_half_limit"]
    return {
        "h1": _mask_case(3, 1, 1, 0, 50, 60, 103, 0),
        "h2_b1000": _mask_case(1000, 2, 1, 2, 28996, 175094, 103, 77),
        "h63": _mask_case(3, 63, 0, 63, 1, (1 << 32) - 1, -5, 5, big_ids=True),
        "h65": _mask_case(3, 65, 65, 10, (1 << 32) - 1, 1, -5, 6, big_ids=True),
        "h100": _mask_case(3, 100, 15, 7, 28996, 175094, (1 << 31) + 7, 0xFFFFFFFF, big_ids=True),
        "h8192": _mask_case(1, limit, int(limit * 0.15), limit, 28996, 175094, 103, 9, big_ids=True),
    }


@functools.lru_cache(maxsize=None)
def mask_expected(name):
    c = mask_cases()[name]
    out = mo.mlm_mask(c["ids"], c["half"], c["vocab_text"], c["vocab_ent"], mask_id=c["mask_id"], k_text=c["k_text"],
                      k_ent=c["k_ent"], seed=c["seed"])
    for a in out:
        a.setflags(write=False)
    return out


def mask_keys(c, b, h):
    """The keys of one half, as the kernel puts them into LDS."""
    rowkey = h32(base_key(c["seed"]) ^ (((b * 2 + h) * mo.K_ROW) & M))
    return np.array([h32((rowkey + pos * mo.K_POS) & M) for pos in range(c["half"])], dtype=np.uint64)


MASK_WRONG = ("rank_le", "tie_ignores_position", "keep_random_swapped")


def mask_model(c, wrong=None):
    """mlm_mask_kernel position by position: rank by COUNTING smaller keys (the restatement sorts), three more hashes.
    wrong: "rank_le" - `rank <= k`; "tie_ignores_position" - equal keys do not count (CANNOT differ: the key map is a
    bijection of the position, see the CPU file); "keep_random_swapped" - the 10 % that keep their id and the 10 % that get a
    random one trade places."""
    ids, half = c["ids"], c["half"]
    B = ids.shape[0]
    out = ids.copy()
    labels = [np.full((B, half), -100, dtype=np.int64), np.full((B, half), -100, dtype=np.int64)]
    pos = np.arange(half)
    for b in range(B):
        for h in range(2):
            keys = mask_keys(c, b, h)
            srt = np.sort(keys)
            rank = np.searchsorted(srt, keys, side="left")                  # keys smaller than mine
            if wrong != "tie_ignores_position":
                first = np.searchsorted(srt, keys, side="left")
                order = np.argsort(keys, kind="stable")
                among = np.empty(half, dtype=np.int64)
                among[order] = np.arange(half) - first[order]               # equal keys at smaller positions
                rank = rank + among
            k = c["k_text"] if h == 0 else c["k_ent"]
            vocab = c["vocab_text"] if h == 0 else c["vocab_ent"]
            chosen = pos[rank <= k] if wrong == "rank_le" else pos[rank < k]
            for p in chosen:
                key, tok = int(keys[p]), int(ids[b, h * half + p])
                keep = (h32(key ^ mo.K_D2) >> 8) < 8388608
                if wrong == "keep_random_swapped":
                    keep = not keep
                if (h32(key ^ mo.K_D1) >> 8) < 13421773:
                    new = c["mask_id"]
                elif keep:
                    new = tok
                else:
                    new = (h32(key ^ mo.K_D3) * vocab) >> 32
                out[b, h * half + p] = new
                labels[h][b, p] = tok
    return out, labels[0], labels[1]


def mask_invariants(c, outs):
    """From the outputs and the inputs alone: exactly k labels per half; a label is the original id where the position was
    chosen and -100 elsewhere; an unchosen id is untouched; a chosen one is the mask id, the original or below the
    vocabulary."""
    ids, half = c["ids"], c["half"]
    out, tl, el = (np.asarray(a) for a in outs)
    assert out.dtype == np.int64 and out.shape == ids.shape and tl.shape == el.shape == (ids.shape[0], half)
    for lab, off, k, vocab in ((tl, 0, c["k_text"], c["vocab_text"]), (el, half, c["k_ent"], c["vocab_ent"])):
        orig, new = ids[:, off:off + half], out[:, off:off + half]
        sel = lab != -100
        assert (sel.sum(axis=1) == k).all(), "not exactly k labels per half"
        assert np.array_equal(lab[sel], orig[sel]) and np.array_equal(new[~sel], orig[~sel])
        ok = (new[sel] == c["mask_id"]) | (new[sel] == orig[sel]) | ((new[sel] >= 0) & (new[sel] < vocab))
        assert ok.all(), "a chosen position holds something else"


# ---------------------------------------------------------------------------------------------------------------------
# assembly: cases
# ---------------------------------------------------------------------------------------------------------------------
SEP = 102
FALLBACK_SEEDS = {2: 1, 3: 1}          # B -> the first seed (rate 0.5) with a negative row that draws itself; CPU file
PARTNER_ONLY_SEED = 9                  # B 3, rate 0.5: the first seed that partner_only_rows() accepts
GAP_SEEDS = {0.2: 0x1D92DA6E, 0.1: 0xFF53EB11, 0.999999: 0x7DFD20AF}     # what gap_seed() constructs; CPU file


def _assemble_case(B, half, rate, seed, n_nodes=40, bad=()):
    """Distinct (source, target) pairs and a walk table without repeated rows, so that an entity half names its row.
    bad: ((array, row, node), ...) planted afterwards."""
    W = half // 2 - 1
    rng = np.random.RandomState(half * 11 + B)
    text = rng.randint(1000, 30000, (B, half)).astype(np.int64) + (1 << 33)
    att = (rng.rand(B, half) < 0.7).astype(np.int64) * rng.choice([1, 5], (B, half))
    walks = (np.arange(n_nodes * W, dtype=np.int64).reshape(n_nodes, W) + 1000) * 3 + (1 << 34)
    perm = rng.permutation(n_nodes)
    source, target = perm[:B].astype(np.int64), perm[B:2 * B].astype(np.int64)
    for which, row, node in bad:
        (source if which == "source" else target)[row] = node
    return dict(text=text, att=att, source=source, target=target, walks=walks, half=half, rate=rate, seed=seed, bad=bool(bad))


def find_fallback_seed(B, rate=0.5):
    """The first seed for which some row is a negative AND draws itself as partner."""
    thr = thr_float(rate)
    seed = 0
    while not any(neg_draw(seed, b) < thr and partner_draw(seed, b, B) == b for b in range(B)):
        seed += 1
    return seed


def assemble_rows_of(c):
    """[(negative, drawn partner, partner used)] per row, by the kernel's rule on Python ints."""
    B = c["text"].shape[0]
    thr = thr_float(c["rate"])
    out = []
    for b in range(B):
        neg = B > 1 and neg_draw(c["seed"], b) < thr
        drawn = partner_draw(c["seed"], b, B) if neg else b
        out.append((neg, drawn, (b + 1) % B if neg and drawn == b else drawn))
    return out


def partner_only_rows(seed=PARTNER_ONLY_SEED, B=3, rate=0.5):
    """(r, readers): a row r that is a negative itself - it never reads its own nodes - and whose nodes are read by the
    negatives `readers` that take r as partner; None if the seed has no such row."""
    c = dict(text=np.zeros((B, 4)), rate=rate, seed=seed)
    rows = assemble_rows_of(c)
    for r in range(B):
        readers = [b for b in range(B) if rows[b][0] and rows[b][2] == r]
        if rows[r][0] and readers:
            return r, readers
    return None


def find_partner_only_seed(B=3, rate=0.5):
    seed = 0
    while partner_only_rows(seed, B, rate) is None:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def assemble_cases():
    """name -> dict(text, att [B, half], source, target [B], walks [n_nodes, W], half, rate, seed, bad). What each owns:
      b1              B = 1 at rate 0.99: never a negative
      fallback_b2/b3  a seed (found on the CPU) for which a negative row draws ITSELF: `(b + 1) % B`
      rate0           threshold 0: no negatives at all
      gap_02/01/1     rate 0.2 / 0.1 / 0.999999 with a seed CONSTRUCTED so that row 1's draw lies between the threshold of
                      the ABI's float and the one of the Python double
      h4, h128, h100  the smallest half (walk_len 1: B S = 24, one partial block), 128, and 100 (B S = 600: two full
                      blocks and a partial one)
      bad_source, bad_target      node = n_nodes in source / node = -1 in target of a row that is read
      bad_partner     a bad source reached ONLY through a negative's partner row (the row itself is a negative too)"""
    c = {}
    c["b1"] = _assemble_case(1, 4, 0.99, 3)
    c["fallback_b2"] = _assemble_case(2, 8, 0.5, FALLBACK_SEEDS[2])
    c["fallback_b3"] = _assemble_case(3, 8, 0.5, FALLBACK_SEEDS[3])
    c["rate0"] = _assemble_case(5, 8, 0.0, 1)
    for name, rate in (("gap_02", 0.2), ("gap_01", 0.1), ("gap_1", 0.999999)):
        c[name] = _assemble_case(3, 8, rate, gap_seed(rate)[0])
    c["h4"] = _assemble_case(3, 4, 0.5, 11)
    c["h128"] = _assemble_case(3, 128, 0.5, 12)
    c["h100"] = _assemble_case(3, 100, 0.5, 13)
    c["bad_source"] = _assemble_case(3, 8, 0.0, 1, bad=(("source", 1, 40),))
    c["bad_target"] = _assemble_case(3, 8, 0.0, 1, bad=(("target", 2, -1),))
    r, _ = partner_only_rows()
    c["bad_partner"] = _assemble_case(3, 8, 0.5, PARTNER_ONLY_SEED, bad=(("source", r, 40),))
    for case in c.values():
        for a in case.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def assemble_expected(name):
    """(ids, attention, types, nsp, error bit) of the restatement."""
    c = assemble_cases()[name]
    return mo.assemble_rows(c["text"], c["att"], c["source"], c["target"], c["walks"], sep_id=SEP, negative_rate=c["rate"],
                            seed=c["seed"], return_err=True)


ASSEMBLE_WRONG = ("thr_double", "second_ge", "fallback_keeps_b", "bad_as_sep")


def assemble_model(c, wrong=None):
    """assemble_kernel element by element. wrong: "thr_double" - the old threshold rule; "second_ge" - the target's walk
    from `e >= walk_len` on (CANNOT differ: e == walk_len is [SEP] before the test is reached); "fallback_keeps_b" - a
    negative that draws itself keeps its own entity half; "bad_as_sep" - a bad node writes sep_id."""
    text, att, walks, half = c["text"], c["att"], c["walks"], c["half"]
    B, S, W, n_nodes = text.shape[0], 2 * half, walks.shape[1], walks.shape[0]
    thr = thr_double(c["rate"]) if wrong == "thr_double" else thr_float(c["rate"])
    ids, at, ty = (np.full((B, S), UNWRITTEN, dtype=np.int64) for _ in range(3))
    nsp, err = np.full(B, UNWRITTEN, dtype=np.int64), 0
    for gid in range(B * S):
        b, p = divmod(gid, S)
        neg = B > 1 and neg_draw(c["seed"], b) < thr
        row = b
        if neg:
            row = partner_draw(c["seed"], b, B)
            if row == b and wrong != "fallback_keeps_b":
                row = (b + 1) % B
        if p == 0:
            nsp[b] = 1 if neg else 0
        if p < half:
            ids[b, p], at[b, p], ty[b, p] = text[b, p], att[b, p], 0
            continue
        e, v = p - half, SEP
        if e != W and e != 2 * W + 1:
            second = e >= W if wrong == "second_ge" else e > W
            node = int(c["target"][row] if second else c["source"][row])
            if node < 0 or node >= n_nodes:
                err |= 1
                v = SEP if wrong == "bad_as_sep" else 0
            else:
                v = walks[node, e - W - 1 if second else e]
        ids[b, p], at[b, p], ty[b, p] = v, 1, 1
    return ids, at, ty, nsp, err


def assemble_invariants(c, outs):
    """From the outputs and the inputs alone (cases without a bad node): the text half and its attention are copied,
    entity-half attention and token type are 1, [SEP] sits at walk_len and 2 walk_len + 1, and nsp == 1 iff the entity
    half is ANOTHER row's (the cases' pairs and walks are distinct, so a half names its row)."""
    assert not c["bad"]
    text, att, walks, half = c["text"], c["att"], c["walks"], c["half"]
    B, W = text.shape[0], walks.shape[1]
    ids, at, ty, nsp = (np.asarray(a) for a in outs[:4])
    assert ids.shape == at.shape == ty.shape == (B, 2 * half) and nsp.shape == (B,)
    assert np.array_equal(ids[:, :half], text) and np.array_equal(at[:, :half], att)
    assert (ty[:, :half] == 0).all() and (ty[:, half:] == 1).all() and (at[:, half:] == 1).all()
    assert (ids[:, half + W] == SEP).all() and (ids[:, half + 2 * W + 1] == SEP).all()
    halves = [np.concatenate([walks[c["source"][r]], [SEP], walks[c["target"][r]], [SEP]]) for r in range(B)]
    for b in range(B):
        whose = [r for r in range(B) if np.array_equal(ids[b, half:], halves[r])]
        assert len(whose) == 1, "an entity half that is no row's"
        assert nsp[b] in (0, 1) and (nsp[b] == 1) == (whose[0] != b), "nsp == 1 iff the entity half is the partner's"


def same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
