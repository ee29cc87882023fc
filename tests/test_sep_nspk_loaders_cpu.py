"""CPU: the separator's geometry is read from a checkpoint's tensor shapes (weights.sep_dims_from_state_dict) and its savedir can be
chosen (find_sepformer_checkpoint `subdir`, build_state_dicts / load_models `sep_checkpoint`).  The checkpoints are written here in
the SpeechBrain savedir layout -- encoder.ckpt, masknet.ckpt, decoder.ckpt, each the state_dict of its module -- for two and for
three speakers; nothing needs a device."""
import inspect

import pytest
import torch

from clearconverse_amd import models
from clearconverse_amd.weights import SepDims, find_sepformer_checkpoint, sep_dims_from_state_dict, synthetic_sepformer_state_dict


def _write_savedir(root, name, dims, seed=3):
    sd = synthetic_sepformer_state_dict(dims, seed=seed)
    d = root / name
    d.mkdir(parents=True)
    for part in ("encoder", "masknet", "decoder"):
        torch.save({k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(part + ".")}, d / f"{part}.ckpt")
    return sd


def test_two_speaker_layout_is_the_default_geometry():
    assert sep_dims_from_state_dict(synthetic_sepformer_state_dict(SepDims(), seed=1)) == SepDims()


@pytest.mark.parametrize("dims", [SepDims(n_spk=3), SepDims(n_spk=1, n_layers=2), SepDims(n_spk=4, n_layers=3, n_blocks=3, d_ffn=256)])
def test_geometry_is_read_from_the_shapes(dims):
    got = sep_dims_from_state_dict(synthetic_sepformer_state_dict(dims, seed=2))
    assert got == dims
    assert (got.n_head, got.stride, got.segment) == (SepDims().n_head, SepDims().stride, SepDims().segment)     # not in the weights


def test_not_a_sepformer_state_dict_is_an_error():
    sd = synthetic_sepformer_state_dict(SepDims(n_layers=1), seed=2)
    bad = dict(sd)
    bad["masknet.model.output_fc.1.weight"] = torch.zeros(128 * 2 + 5, 128, 1)
    with pytest.raises(ValueError, match="output_fc"):
        sep_dims_from_state_dict(bad)
    with pytest.raises(ValueError, match="seg_model"):
        sep_dims_from_state_dict({k: v for k, v in sd.items() if "seg_model" not in k})


def test_savedir_can_be_chosen(tmp_path):
    two = _write_savedir(tmp_path, "resepformer", SepDims(n_layers=1))
    three = _write_savedir(tmp_path, "resepformer-wsj03mix", SepDims(n_layers=1, n_spk=3), seed=5)
    default = find_sepformer_checkpoint(str(tmp_path))
    assert sorted(default) == sorted(two) and all(torch.equal(default[k], two[k]) for k in two)
    got = find_sepformer_checkpoint(str(tmp_path), subdir="resepformer-wsj03mix")
    assert sorted(got) == sorted(three) and all(torch.equal(got[k], three[k]) for k in three)
    assert sep_dims_from_state_dict(got) == SepDims(n_layers=1, n_spk=3) and sep_dims_from_state_dict(default) == SepDims(n_layers=1)
    assert find_sepformer_checkpoint(str(tmp_path), subdir="resepformer-wsj04mix") is None
    # the fine-tune overlay rule is unchanged: its directory is `resepformer-ft` whatever the base, shape mismatches are skipped
    ft = _write_savedir(tmp_path, "resepformer-ft", SepDims(n_layers=1), seed=8)
    (tmp_path / "resepformer-ft" / "hyperparams.yaml").write_text("{}\n")
    over = find_sepformer_checkpoint(str(tmp_path), apply_ft_overlay=True, subdir="resepformer-wsj03mix")
    assert torch.equal(over["encoder.conv1d.weight"], ft["encoder.conv1d.weight"])
    assert torch.equal(over["masknet.model.output_fc.1.weight"], three["masknet.model.output_fc.1.weight"])
    kept = find_sepformer_checkpoint(str(tmp_path), subdir="resepformer-wsj03mix")
    assert torch.equal(kept["encoder.conv1d.weight"], three["encoder.conv1d.weight"])


def _light_build(monkeypatch, tmp_path):
    """build_state_dicts with every other network's generator stubbed out: only the separator's branch is under test"""
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("CCX_APPLY_RESEPFORMER_FT", raising=False)
    for name in ("synthetic_whisper_state_dict", "synthetic_xvector_state_dict", "synthetic_pyannet_state_dict",
                 "synthetic_resnet34_state_dict"):
        monkeypatch.setattr(models, name, lambda *a, **k: {})
    monkeypatch.setattr(models, "find_pyannote_checkpoint", lambda kind: None)
    monkeypatch.setattr(models, "find_whisper_checkpoint", lambda size: None)


def test_build_state_dicts_takes_the_checkpoints_geometry(monkeypatch, tmp_path):
    _light_build(monkeypatch, tmp_path)
    three = _write_savedir(tmp_path, "resepformer-wsj03mix", SepDims(n_layers=1, n_spk=3), seed=5)
    W = models.build_state_dicts(sep_checkpoint="resepformer-wsj03mix")
    assert SepDims(**W["sep_dims"]) == SepDims(n_layers=1, n_spk=3) and W["weights_sources"]["sepformer"] == "checkpoint"
    assert all(torch.equal(W["sepformer"][k], three[k]) for k in three)
    # the default savedir is absent here: synthetic weights of the default geometry, as before
    W = models.build_state_dicts()
    assert SepDims(**W["sep_dims"]) == SepDims() and W["weights_sources"]["sepformer"].startswith("synthetic")
    # an explicit geometry still means synthetic weights of that geometry
    W = models.build_state_dicts(sep_dims=SepDims(n_layers=1, n_spk=3), sep_checkpoint="resepformer-wsj03mix")
    assert W["weights_sources"]["sepformer"].startswith("synthetic") and W["sepformer"]["masknet.model.output_fc.1.weight"].shape[0] == 384
    _write_savedir(tmp_path, "resepformer", SepDims(n_layers=1))
    W = models.build_state_dicts()
    assert SepDims(**W["sep_dims"]) == SepDims(n_layers=1) and W["weights_sources"]["sepformer"] == "checkpoint"


def test_load_models_hands_the_savedir_on_and_refuses_contradicting_dims(monkeypatch):
    assert inspect.signature(models.load_models).parameters["sep_checkpoint"].default == "resepformer"
    assert inspect.signature(models.build_state_dicts).parameters["sep_checkpoint"].default == "resepformer"
    assert inspect.signature(find_sepformer_checkpoint).parameters["subdir"].default == "resepformer"
    monkeypatch.setattr(models.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(models._lib, "Context", lambda dev: object())
    seen = {}

    def fake_build(config, whisper_dims, sep_dims, seed, embedding="xvector", sep_checkpoint="resepformer"):
        seen["sep_checkpoint"] = sep_checkpoint
        raise RuntimeError("stop here")
    monkeypatch.setattr(models, "build_state_dicts", fake_build)
    with pytest.raises(RuntimeError, match="stop here"):
        models.load_models(sep_checkpoint="resepformer-wsj03mix")
    assert seen == {"sep_checkpoint": "resepformer-wsj03mix"}
    # the geometry travels with the weights: a contradicting sep_dims is an error, before any model is built
    W = {"whisper_dims": dict(models.WhisperDims.mini().__dict__), "whisper": {}, "sep_dims": dict(SepDims(n_spk=3).__dict__), "sepformer": {}}
    with pytest.raises(ValueError, match="sep_dims"):
        models.load_models(state_dicts=W, sep_dims=SepDims())
    with pytest.raises(ValueError, match="sep_dims"):
        models.load_models(state_dicts=dict(W, sep_dims=dict(SepDims().__dict__)), sep_dims=SepDims(n_spk=3))
