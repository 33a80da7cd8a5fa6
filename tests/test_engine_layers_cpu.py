"""The layering of the engines: `layer_engine.LayerEngine` is the model-independent core (workspace, streams, GEMM and
weight-gradient wrappers, derived weights, one BERT layer), `engine.Engine` puts STonKGs' front and heads around it, and
`bigbird_encoder.BigBirdEngine` builds on the core alone - it carries nothing of STonKGs."""
import pytest

from stonkgs_amd import bigbird_encoder, engine, layer_engine
from stonkgs_amd.bigbird_encoder import BigBirdEncoderConfig, BigBirdEngine
from stonkgs_amd.engine import Engine, TextEngine
from stonkgs_amd.layer_engine import LayerEngine

STONKGS_ONLY = ("backbone_fwd", "prefetch_backbone", "special_vectors", "_plan_rows", "encode", "forward", "backward", "evaluate",
                "attention_maps", "input_gradients", "forward_cls", "backward_cls")
# what FlatBufferModel, FusedAdamW and Trainer call on any engine
ANY_ENGINE = ("refresh_derived", "adamw_tables", "optimizer_stream", "wait_params", "take_wgrad_sumsq", "check_errors",
              "join_wgrad", "block", "layer_fwd", "layer_bwd")
CONSTANTS = {"ERR_BITS", "KEY_ERROR_BITS"}
STORE_HOOK = "_mirrored_stores"     # the stores whose bf16 mirror refresh_derived casts: the one documented override


def test_bigbird_engine_is_a_layer_engine_and_no_stonkgs_engine():
    assert issubclass(BigBirdEngine, LayerEngine) and not issubclass(BigBirdEngine, Engine)
    assert issubclass(Engine, LayerEngine) and issubclass(TextEngine, Engine)


@pytest.mark.parametrize("cls", [LayerEngine, BigBirdEngine])
def test_the_core_has_none_of_stonkgs_methods(cls):
    assert [n for n in STONKGS_ONLY if hasattr(cls, n)] == []


def test_the_core_has_what_model_optimizer_and_trainer_call():
    assert [n for n in ANY_ENGINE if not callable(vars(LayerEngine).get(n))] == []
    assert [n for n in ("_attention_fwd", "_attention_bwd", "_ffn_up", "_ffn_down_dgrad") if n not in vars(LayerEngine)] == []


def test_nothing_was_left_behind_as_a_copy():
    shared = set(vars(Engine)) & set(vars(LayerEngine))
    plain = {n for n in shared if not (n.startswith("__") and n.endswith("__"))}
    assert "__init__" in shared
    assert plain <= CONSTANTS | {STORE_HOOK}, plain
    assert LayerEngine._mirrored_stores.__doc__     # (documented)
    # ... and BigBirdEngine replaces the four layer methods, its constants and the constructor, nothing else of the core
    over = {n for n in set(vars(BigBirdEngine)) & set(vars(LayerEngine)) if not (n.startswith("__") and n.endswith("__"))}
    assert over == CONSTANTS | {"_attention_fwd", "_attention_bwd", "_ffn_up", "_ffn_down_dgrad"}, over


def test_engine_exports_every_name_it_exported():
    for name in ("Engine", "TextEngine", "GemmTimer", "Rows", "ReadRows", "padded_rows", "decoders", "Decoder", "ERR_BITS",
                 "TEXT_ERR_BITS", "BF16", "F32", "I32"):
        assert hasattr(engine, name), name
        if hasattr(layer_engine, name):
            assert getattr(engine, name) is getattr(layer_engine, name), name
    for name in ("GemmTimer", "Rows", "ReadRows", "padded_rows"):   # what moved with the core is DEFINED there
        assert getattr(engine, name).__module__ == "stonkgs_amd.layer_engine", name
    assert bigbird_encoder.LayerEngine is LayerEngine


def test_a_bigbird_engine_instance_carries_nothing_of_stonkgs():
    """The constructors launch nothing, so they run on the CPU; they need the built library."""
    from stonkgs_amd.params import FlatStore, trainable_specs

    cfg = BigBirdEncoderConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                               max_position_embeddings=1024)
    eng = BigBirdEngine(cfg, FlatStore(trainable_specs(cfg, False), "cpu", trainable=True), "cpu")
    assert [n for n in ("BB", "kg_table", "rows_executed", "next_input_ids", "unpad", "saved") if hasattr(eng, n)] == []
    assert [n for n in STONKGS_ONLY if hasattr(eng, n)] == []
    assert eng.ERR_BITS is BigBirdEngine.ERR_BITS and eng._mirrored_stores() == (eng.P,)
    print("attributes of a BigBirdEngine instance:", len(vars(eng)))
