"""CPU: the ECAPA-TDNN checkpoint loader (clearconverse_amd.weights.find_ecapa_checkpoint) and the `embedding=` option of
clearconverse_amd.models: a self-written `embedding_model.ckpt` in the hub layout is found and conformed; a missing key, a permuted
shape and a pickled object are refused loudly; an unknown embedder name raises."""
import os

import pytest
import torch

from clearconverse_amd import weights as W


class _Pickled:
    pass


def _write(root, sd, layout="hub"):
    if layout == "hub":
        d = os.path.join(root, "ecapa", "models--speechbrain--spkrec-ecapa-voxceleb", "snapshots", "abc123")
    else:
        d = os.path.join(root, "speechbrain", "spkrec-ecapa-voxceleb")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "embedding_model.ckpt")
    torch.save(sd, path)
    return path


@pytest.fixture(scope="module")
def schema():
    return W.synthetic_ecapa_state_dict(seed=9)


def test_schema_has_the_speechbrain_key_layout(schema):
    for k, shape in (("blocks.0.conv.conv.weight", (1024, 80, 5)), ("blocks.2.res2net_block.blocks.6.norm.norm.running_var", (128,)),
                     ("blocks.3.res2net_block.blocks.0.conv.conv.weight", (128, 128, 3)), ("blocks.1.se_block.conv1.conv.weight", (128, 1024, 1)),
                     ("blocks.1.se_block.conv2.conv.bias", (1024,)), ("mfa.conv.conv.weight", (3072, 3072, 1)),
                     ("asp.tdnn.conv.conv.weight", (128, 9216, 1)), ("asp.conv.conv.weight", (3072, 128, 1)),
                     ("asp_bn.norm.running_mean", (6144,)), ("fc.conv.weight", (192, 6144, 1)), ("fc.conv.bias", (192,))):
        assert tuple(schema[k].shape) == shape, k
    assert len(schema) == 6 + 3 * (2 * 6 + 7 * 6 + 4) + 6 + 6 + 2 + 4 + 2


@pytest.mark.parametrize("layout", ["hub", "plain"])
def test_checkpoint_is_found_and_conformed(tmp_path, schema, layout):
    sd = {k: v.clone() for k, v in schema.items()}
    sd["blocks.0.norm.norm.num_batches_tracked"] = torch.tensor(7)            # extra keys of a real checkpoint are dropped
    sd["fc.conv.bias"] = sd["fc.conv.bias"].double()                          # widened / narrowed to f32
    _write(str(tmp_path), sd, layout)
    got = W.find_ecapa_checkpoint(cache_dir=str(tmp_path))
    assert got is not None and set(got) == set(schema)
    assert all(torch.equal(got[k].float(), schema[k]) for k in schema)
    assert W.find_ecapa_checkpoint(cache_dir=str(tmp_path / "nothing_here")) is None


def test_missing_key_and_permuted_shape_are_refused(tmp_path, schema):
    sd = {k: v for k, v in schema.items() if k != "asp.conv.conv.bias"}
    _write(str(tmp_path / "a"), sd)
    with pytest.raises(ValueError, match="asp.conv.conv.bias"):
        W.find_ecapa_checkpoint(cache_dir=str(tmp_path / "a"))
    sd = dict(schema)
    sd["blocks.1.res2net_block.blocks.0.conv.conv.weight"] = sd["blocks.1.res2net_block.blocks.0.conv.conv.weight"].permute(2, 1, 0).contiguous()
    _write(str(tmp_path / "b"), sd)
    with pytest.raises(ValueError, match="shape"):
        W.find_ecapa_checkpoint(cache_dir=str(tmp_path / "b"))


def test_pickled_object_is_refused(tmp_path, schema):
    path = _write(str(tmp_path), {"state": _Pickled(), **schema})
    with pytest.raises(W.CheckpointRefused, match="weights-only"):
        W.load_state_dict_file(path)
    said = []
    assert W.find_ecapa_checkpoint(cache_dir=str(tmp_path), log=said.append) is None      # nothing is executed; the caller is told
    assert said and "refused" in said[0] and "ecapa" in said[0]


def test_unknown_embedding_name_raises():
    from clearconverse_amd.models import build_state_dicts, load_models
    with pytest.raises(ValueError, match="bogus"):
        load_models(embedding="bogus")
    with pytest.raises(ValueError, match="bogus"):
        build_state_dicts(embedding="bogus")


def test_fbank_tables_shapes():
    tb = W.ecapa_fbank_tables()
    assert tuple(tb["fbank.window"].shape) == (400,) and tuple(tb["fbank.filters"].shape) == (80, 201)
    assert tb["fbank.filters"].dtype == torch.float32 and float(tb["fbank.filters"].min()) == 0.0 and float(tb["fbank.filters"].max()) <= 1.0
