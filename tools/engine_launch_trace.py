"""What the engines ask of the kernel library, call by call: a recording proxy in front of the loaded library handle
(`_hip._lib`) writes one line per C-ABI call, and the calls that order streams (`Stream.wait_stream`, `Stream.wait_event`,
`Event.record`) are logged between them, in program order. Two versions of the host code that write the same trace issue
the same launches with the same arguments in the same stream order - what a refactor of the engines has to show.

    python tools/engine_launch_trace.py PACKAGE_ROOT OUT_FILE [SCENARIO ...]

PACKAGE_ROOT: the directory that holds the `stonkgs_amd/` package to trace - this checkout, or a copy of another commit's
Python package (the library itself comes from STONK_HIP_LIB or from that package's csrc/). OUT_FILE: the trace; its line
count and sha256 are printed. Needs the GPU.

A line: the entry's name, then every argument - a non-pointer argument literally, a pointer (the stream included) as `p<n>`,
n = the position of its first appearance in the trace (null stays `null`), the members of a TnProblem array spelled out the
same way - then the value returned. Streams and events in the ordering lines are numbered the same way (`p<n>`: a stream is
its handle; `e<n>`: events, by object).

Scenarios (fixed seeds, the smallest configurations the kernels accept; each takes under a second on an MI355X, `store` with
its large decoders included - the wall time of each is printed to stderr). STonKGs: hidden 128, 2 layers,
2 heads, S 256, B 3 (the shape of tests/golden/g2_hipsmall). BigBird: hidden 128, 2 layers, S 768 (the shortest length above
the full-attention threshold), B 1.
  pretrain      two Trainer.training_step at dropout 0.1 with the next batch hinted (prefetch miss, then hit): the packed
                layout; store mode asks, and accumulates (the routing splits K at this shape)
  eval_dense    an eval-mode forward with dense logits: the padded layout
  detached      evaluate_batch and attention_maps between a training forward and its backward; input_attributions refuses
                to run there (it uses that forward's buffers: the refusal is logged) and runs behind the backward
  comm_overlap  one forward_backward with `comm_overlap` set by hand
  gemm_timer    one Trainer step with a GemmTimer attached
  cls           STonKGsForSequenceClassification.forward_backward: cross-entropy, then a regression (MSE) model
  text          one Trainer step of BertForSequenceClassification (TextEngine)
  bigbird       BigBirdEncoderModel: forward + backward in .train(), and a no-grad forward
  wide          one Trainer step at hidden 256 / intermediate 1024 / 3 layers / B 8 with `tn_min_k`, `tn_min_tiles` lowered:
                the grouped attention weight gradients (no smaller shape reaches the four-wave weight-gradient kernel)
  store         two Trainer steps of the small model with 31 000 tokens and 62 000 entities: both decoders' gradients leave
                unsplit, so they are stored with their sum-of-squares slots and the optimizer takes its norm from them
"""
import ctypes
import gc
import hashlib
import os
import sys
import time

import torch

SMALL = dict(vocab_size=512, kg_vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
             intermediate_size=256, max_position_embeddings=256)
WIDE = dict(vocab_size=2048, kg_vocab_size=512, hidden_size=256, num_hidden_layers=3, num_attention_heads=4,
            intermediate_size=1024, max_position_embeddings=256)
B, S = 3, 256


class Trace:
    def __init__(self):
        self.lines = []
        self.ptrs = {}      # address -> index of first appearance
        self.events = {}    # id(event) -> (index, the event: kept alive so that the id stays its own)

    def ptr(self, p) -> str:
        p = getattr(p, "value", p) or 0
        return "null" if p == 0 else f"p{self.ptrs.setdefault(int(p), len(self.ptrs))}"

    def event(self, e) -> str:
        return f"e{self.events.setdefault(id(e), (len(self.events), e))[0]}"

    def arg(self, a, ctype) -> str:
        if isinstance(a, ctypes.Array):   # a host array of TnProblem
            return "[" + " ".join("{" + ",".join(f"{n}={self.arg(getattr(q, n), t)}" for n, t in q._fields_) + "}" for q in a) + "]"
        if ctype is ctypes.c_void_p:
            return self.ptr(a)
        return repr(float(a)) if ctype in (ctypes.c_float, ctypes.c_double) else repr(int(a))

    def say(self, *words) -> None:
        self.lines.append(" ".join(words))


class Recorder:
    """Stands where the library handle stood: every function looked up on it is called through, and written down."""

    def __init__(self, handle, trace: Trace):
        self._handle, self._trace, self._fns = handle, trace, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real, t = getattr(self._handle, name), self._trace

            def fn(*args):
                types = real.argtypes or ()
                if len(types) != len(args):
                    raise TypeError(f"{name}: {len(args)} arguments for {len(types)} declared")
                words = [t.arg(a, c) for a, c in zip(args, types)]   # (numbered before the call: first APPEARANCE)
                rc = real(*args)
                t.say(name, *words, "->", repr(rc))
                return rc

            self._fns[name] = fn
        return fn


def log_stream_order(trace: Trace) -> None:
    Stream, Event = torch.cuda.Stream, torch.cuda.Event
    wait_stream, wait_event, record = Stream.wait_stream, Stream.wait_event, Event.record

    def _wait_stream(self, other):
        trace.say("Stream.wait_stream", trace.ptr(self.cuda_stream), trace.ptr(other.cuda_stream))
        return wait_stream(self, other)

    def _wait_event(self, event):
        trace.say("Stream.wait_event", trace.ptr(self.cuda_stream), trace.event(event))
        return wait_event(self, event)

    def _record(self, stream=None):
        s = torch.cuda.current_stream() if stream is None else stream
        trace.say("Event.record", trace.event(self), trace.ptr(s.cuda_stream))
        return record(self, stream)

    Stream.wait_stream, Stream.wait_event, Event.record = _wait_stream, _wait_event, _record


# ------------------------------------------------------------------------------------------------ scenarios
def _config(dims, p, **kw):
    from stonkgs_amd.config import STonKGsConfig

    return STonKGsConfig(**dims, hidden_dropout_prob=p, attention_probs_dropout_prob=p, **kw)


def _table(dims, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(dims["kg_vocab_size"], dims["hidden_size"], generator=g, dtype=torch.float64) * 0.3


def _pretraining(dims=SMALL, p=0.1):
    from stonkgs_amd.stonkgs_model import STonKGsForPreTraining

    return STonKGsForPreTraining(_config(dims, p), kg_embeddings=_table(dims, 8), seed=3)


def _batch(seed, dims=SMALL, b=B):
    from stonkgs_amd.data import synthetic_batch

    batch = synthetic_batch(b, dims["vocab_size"], dims["kg_vocab_size"], S, seed=seed, min_text=16)
    return {k: v.cuda() for k, v in batch.items()}


def _trainer(model, **kw):
    from stonkgs_amd.stonkgs_pretraining import Trainer, TrainingArguments

    return Trainer(model, TrainingArguments(max_steps=10, learning_rate=1e-3, per_device_train_batch_size=B, **kw))


KEEP = []   # every model stays alive to the end: no address is handed out twice because a scenario's memory was freed


def _done(model) -> None:
    model.engine.join_wgrad()
    torch.cuda.synchronize()
    model.engine.check_errors()
    KEEP.append(model)


def pretrain(trace):
    model = _pretraining()
    tr, batches = _trainer(model), [_batch(20), _batch(21)]
    tr.training_step(model, batches[0], next_inputs=batches[1])   # nothing was prefetched for it: a miss, then the hint
    tr.training_step(model, batches[1])                           # a hit
    _done(model)


def eval_dense(trace):
    model = _pretraining()
    model.eval()
    with torch.no_grad():
        model(**_batch(20))
    _done(model)


def detached(trace):
    model = _pretraining()
    model.train()
    batch = _batch(20)
    inputs = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    labels = {k: batch[k] for k in ("masked_lm_labels", "ent_masked_lm_labels", "next_sentence_labels")}
    loss = model(**batch)[0]
    model.evaluate_batch(batch, k=10)
    model.attention_maps(**inputs, layers=[0, 1])
    try:
        model.input_attributions(**inputs, labels=labels)
    except RuntimeError:
        trace.say("input_attributions refused: a forward is waiting for its backward")
    loss.backward()
    model.input_attributions(**inputs, labels=labels)
    _done(model)


def comm_overlap(trace):
    model = _pretraining()
    model.train()
    model.engine.comm_overlap = True
    model.forward_backward(_batch(20))
    _done(model)


def gemm_timer(trace):
    from stonkgs_amd.engine import GemmTimer

    model = _pretraining()
    model.engine.gemm_timer = GemmTimer()
    _trainer(model).training_step(model, _batch(20))
    _done(model)


def cls(trace):
    from stonkgs_amd.stonkgs_model import STonKGsForSequenceClassification

    batch = {k: v for k, v in _batch(20).items() if k in ("input_ids", "attention_mask", "token_type_ids")}
    g = torch.Generator().manual_seed(5)
    for labels, problem in ((torch.randint(0, 3, (B,), generator=g), None), (torch.randn(B, 3, generator=g), "regression")):
        model = STonKGsForSequenceClassification(_config(SMALL, 0.1, num_labels=3), kg_embeddings=_table(SMALL, 8), seed=3)
        model.config.problem_type = problem
        model.train()
        model.forward_backward(dict(batch, labels=labels))
        _done(model)


def text(trace):
    from stonkgs_amd.nlp_baseline_model import BertForSequenceClassification

    dims = {k: v for k, v in SMALL.items() if k != "kg_vocab_size"}
    model = BertForSequenceClassification(_config(dims, 0.1), num_labels=3)
    g = torch.Generator().manual_seed(5)
    ids, am = torch.zeros(B, S, dtype=torch.long), torch.zeros(B, S, dtype=torch.long)
    for b, n in enumerate((1, 100, 256)):
        ids[b, :n], am[b, :n] = torch.randint(1, dims["vocab_size"], (n,), generator=g), 1
    batch = dict(input_ids=ids, attention_mask=am, token_type_ids=torch.zeros_like(ids), labels=torch.randint(0, 3, (B,), generator=g))
    _trainer(model).training_step(model, batch)
    _done(model)


def bigbird(trace):
    from stonkgs_amd.bigbird_encoder import BigBirdEncoderConfig, BigBirdEncoderModel

    cfg = BigBirdEncoderConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                               max_position_embeddings=1024)
    model = BigBirdEncoderModel(cfg, seed=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 768, 128, generator=g).cuda().requires_grad_(True)
    mask = torch.ones(1, 768, dtype=torch.long)
    mask[:, 700:] = 0
    model.train()
    seq, pooled = model(x, mask.cuda())
    (seq.sum() + pooled.sum()).backward()
    with torch.no_grad():
        model(x.detach(), mask.cuda())
    _done(model)


def wide(trace):
    model = _pretraining(WIDE)
    model.engine.tn_min_k, model.engine.tn_min_tiles = 512, 4
    _trainer(model).training_step(model, _batch(20, WIDE, 8))
    _done(model)


def store(trace):
    dims = dict(SMALL, vocab_size=31000, kg_vocab_size=62000)
    model = _pretraining(dims)
    tr = _trainer(model)
    for seed in (20, 21):
        tr.training_step(model, _batch(seed, dims, 4))
    _done(model)


SCENARIOS = dict(pretrain=pretrain, eval_dense=eval_dense, detached=detached, comm_overlap=comm_overlap, gemm_timer=gemm_timer,
                 cls=cls, text=text, bigbird=bigbird, wide=wide, store=store)


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    root, out, names = os.path.abspath(argv[1]), argv[2], argv[3:] or list(SCENARIOS)
    if not os.path.isdir(os.path.join(root, "stonkgs_amd")):
        raise SystemExit(f"{root} holds no stonkgs_amd/ package")
    if not torch.cuda.is_available():
        raise SystemExit("engine_launch_trace.py needs the GPU: the engines launch what they schedule")
    sys.path.insert(0, root)
    from stonkgs_amd import _hip as hip

    assert os.path.dirname(os.path.abspath(hip.__file__)) == os.path.join(root, "stonkgs_amd"), hip.__file__
    gc.disable()   # (objects die where their last reference goes, in both versions alike: addresses are reused alike)
    trace = Trace()
    hip._lib = Recorder(hip.lib(), trace)
    log_stream_order(trace)
    for name in names:
        trace.say("#", name)
        torch.manual_seed(0)
        t0 = time.perf_counter()
        SCENARIOS[name](trace)
        torch.cuda.synchronize()
        print(f"{name}: {time.perf_counter() - t0:.1f} s", file=sys.stderr)   # (wall time: beside the trace, never in it)
    text_ = "\n".join(trace.lines) + "\n"
    with open(out, "w") as f:
        f.write(text_)
    print(f"{out}: {len(trace.lines)} lines, sha256 {hashlib.sha256(text_.encode()).hexdigest()}")


if __name__ == "__main__":
    main(sys.argv)
