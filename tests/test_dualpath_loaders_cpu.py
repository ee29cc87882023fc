"""CPU: the loaders of the dual-path SepFormer -- family detection by keys, geometry from tensor shapes and key counts, the chunk length
from a savedir's hyperparams.yaml, `pos_enc.pe` buffers carried along, the two refusals by name -- on savedirs written here in
SpeechBrain's layout (no published checkpoint exists offline).  A RE-SepFormer savedir loads exactly as before."""
import hashlib
import json
import os

import pytest
import torch

from clearconverse_amd import models
from clearconverse_amd import weights as W
from clearconverse_amd.weights import (DualPathDims, SepDims, dual_path_dims_from_state_dict, dual_path_segment_from_yaml,
                                       find_separator_checkpoint, find_sepformer_checkpoint, sep_dims_from_state_dict, sepformer_family,
                                       synthetic_dualpath_state_dict, synthetic_sepformer_state_dict)

SMALL = DualPathDims(kernel=8, stride=4, d_ffn=128, n_layers=2, n_blocks=3, n_spk=3)


def _write_savedir(root, name, sd, yaml=None):
    base = os.path.join(str(root), name)
    os.makedirs(base, exist_ok=True)
    for part in ("encoder", "masknet", "decoder"):
        torch.save({k[len(part) + 1:]: v for k, v in sd.items() if k.startswith(part + ".")}, os.path.join(base, f"{part}.ckpt"))
    if yaml is not None:
        with open(os.path.join(base, "hyperparams.yaml"), "w") as f:
            f.write(yaml)
    return base


def test_published_defaults():
    assert DualPathDims() == DualPathDims(n_filters=256, kernel=16, stride=8, d_model=256, n_head=8, d_ffn=1024, n_layers=8, n_blocks=2,
                                          segment=250, n_spk=2)


def test_family_detection_by_keys():
    assert sepformer_family(synthetic_dualpath_state_dict(SMALL, 1)) == "dualpath"
    assert sepformer_family(synthetic_sepformer_state_dict(SepDims(n_layers=1), 1)) == "resepformer"
    with pytest.raises(ValueError, match="not a SepFormer"):
        sepformer_family({"encoder.conv1d.weight": torch.zeros(1)})


def test_geometry_from_shapes_and_key_counts():
    sd = synthetic_dualpath_state_dict(SMALL, 2)
    assert dual_path_dims_from_state_dict(sd) == SMALL
    assert dual_path_dims_from_state_dict(sd, segment=100) == DualPathDims(**dict(SMALL.__dict__, segment=100))
    one = DualPathDims(n_layers=1, n_blocks=1, n_spk=1, d_ffn=64)
    assert dual_path_dims_from_state_dict(synthetic_dualpath_state_dict(one, 3)) == one
    # source-major mask head: n_spk blocks of n_filters rows
    assert sd["masknet.conv2d.weight"].shape == (256 * 3, 256, 1, 1)
    bad = dict(sd)
    bad["masknet.conv2d.weight"] = torch.zeros(256 * 3 - 1, 256, 1, 1)
    with pytest.raises(ValueError, match="no multiple"):
        dual_path_dims_from_state_dict(bad)
    with pytest.raises(ValueError, match="not a dual-path"):
        dual_path_dims_from_state_dict({k: v for k, v in sd.items() if "dual_mdl" not in k})


def test_pos_enc_buffers_are_carried_and_change_nothing():
    sd = synthetic_dualpath_state_dict(SMALL, 2, pos_enc_buffers=True)
    assert any(k.endswith(".pos_enc.pe") for k in sd)
    assert dual_path_dims_from_state_dict(sd) == SMALL
    plain = synthetic_dualpath_state_dict(SMALL, 2)
    assert all(torch.equal(sd[k], plain[k]) for k in plain)


@pytest.mark.parametrize("key,flag", [("masknet.pos_enc.pe", "use_global_pos_enc"),
                                      ("masknet.dual_mdl.0.intra_linear.weight", "linear_layer_after_inter_intra"),
                                      ("masknet.dual_mdl.1.inter_linear.bias", "linear_layer_after_inter_intra")])
def test_the_two_refusals_name_the_tensor(key, flag):
    sd = dict(synthetic_dualpath_state_dict(SMALL, 2), **{key: torch.zeros(4)})
    with pytest.raises(ValueError, match=flag) as e:
        dual_path_dims_from_state_dict(sd)
    assert key in str(e.value)


def test_segment_from_hyperparams_yaml(tmp_path):
    sd = synthetic_dualpath_state_dict(SMALL, 4, pos_enc_buffers=True)
    yaml = "# SepFormer\nN_encoder_out: 256\nkernel_size: 8\n\nMaskNet: !new:speechbrain.lobes.models.dual_path.Dual_Path_Model\n    num_spks: 3\n    K: 120   # chunk\n    norm: ln\n"
    base = _write_savedir(tmp_path, "sepformer-wsj03mix", sd, yaml)
    assert dual_path_segment_from_yaml(base) == 120
    assert dual_path_segment_from_yaml(_write_savedir(tmp_path, "sepformer-wham", sd)) is None
    assert dual_path_segment_from_yaml(_write_savedir(tmp_path, "sepformer-whamr", sd, "num_spks: 2\n")) is None
    fam, got, dims = find_separator_checkpoint(str(tmp_path), "sepformer-wsj03mix")
    assert fam == "dualpath" and dims == DualPathDims(**dict(SMALL.__dict__, segment=120))
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k].float()) for k in sd)
    assert find_separator_checkpoint(str(tmp_path), "sepformer-wham")[2].segment == 250
    assert find_separator_checkpoint(str(tmp_path), "sepformer-libri3mix") is None


def test_resepformer_savedirs_load_as_before(tmp_path):
    sd = synthetic_sepformer_state_dict(SepDims(n_layers=1, n_spk=3), seed=5)
    _write_savedir(tmp_path, "resepformer-wsj03mix", sd)
    flat = find_sepformer_checkpoint(str(tmp_path), subdir="resepformer-wsj03mix")
    assert isinstance(flat, dict) and set(flat) == set(sd) and sep_dims_from_state_dict(flat) == SepDims(n_layers=1, n_spk=3)
    fam, got, dims = find_separator_checkpoint(str(tmp_path), "resepformer-wsj03mix")
    assert fam == "resepformer" and dims == SepDims(n_layers=1, n_spk=3) and set(got) == set(sd)
    # the plain finder hands a dual-path savedir over as it is: one flat dict, the family is in its keys
    _write_savedir(tmp_path, "sepformer-wsj02mix", synthetic_dualpath_state_dict(SMALL, 6))
    assert sepformer_family(find_sepformer_checkpoint(str(tmp_path), subdir="sepformer-wsj02mix")) == "dualpath"


def _stub_other_networks(monkeypatch):
    monkeypatch.setattr(models, "find_whisper_checkpoint", lambda size: None)
    monkeypatch.setattr(models, "synthetic_whisper_state_dict", lambda d, seed=0: {})
    monkeypatch.setattr(models, "find_pyannote_checkpoint", lambda kind: {})
    monkeypatch.setattr(models, "find_pipeline_config", lambda kind: {})


def test_build_state_dicts_picks_the_family(monkeypatch, tmp_path):
    _stub_other_networks(monkeypatch)
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path))
    _write_savedir(tmp_path, "sepformer-wsj03mix", synthetic_dualpath_state_dict(SMALL, 7), "    K: 50\n")
    Wd = models.build_state_dicts(sep_checkpoint="sepformer-wsj03mix")
    assert Wd["sep_family"] == "dualpath" and DualPathDims(**Wd["sep_dims"]) == DualPathDims(**dict(SMALL.__dict__, segment=50))
    assert Wd["weights_sources"]["sepformer"] == "checkpoint" and "masknet.dual_mdl.0.intra_norm.weight" in Wd["sepformer"]
    with pytest.raises(ValueError, match="dual-path"):
        models.build_state_dicts(sep_checkpoint="sepformer-wsj03mix", sep_family="resepformer")
    # no savedir: the defaults are what they were; sep_family="dualpath" asks for seeded weights of the new family
    Wd = models.build_state_dicts()
    assert "sep_family" not in Wd and SepDims(**Wd["sep_dims"]) == SepDims() and "masknet.model.output_fc.0.weight" in Wd["sepformer"]
    small = DualPathDims(n_layers=1, d_ffn=64, segment=10, n_spk=3)
    Wd = models.build_state_dicts(sep_family="dualpath", sep_dims=small)
    assert Wd["sep_family"] == "dualpath" and DualPathDims(**Wd["sep_dims"]) == small
    assert Wd["sepformer"]["masknet.conv2d.weight"].shape[0] == 3 * 256 and Wd["weights_sources"]["sepformer"].startswith("synthetic")
    again = models.build_state_dicts(sep_family="dualpath", sep_dims=small)
    assert all(torch.equal(Wd["sepformer"][k], again["sepformer"][k]) for k in Wd["sepformer"])
    with pytest.raises(ValueError, match="DualPathDims"):
        models.build_state_dicts(sep_family="dualpath", sep_dims=SepDims())
    with pytest.raises(ValueError, match="sep_family"):
        models.build_state_dicts(sep_family="dprnn")
    assert W.DualPathDims is DualPathDims


def test_synthetic_separator_weights_keep_their_bits():
    """The seeded state dicts of both families (seed 1 of the default RE-SepFormer is the benchmark's) against digests recorded before
    the per-layer keys moved into one helper: sha256 over every key, in order, followed by its tensor's bytes."""
    def digest(sd):
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode())
            h.update(v.detach().contiguous().numpy().tobytes())
        return h.hexdigest()

    with open(os.path.join(os.path.dirname(__file__), "golden", "synthetic_separator_digests.json")) as f:
        want = json.load(f)
    got = {
        "sepformer_default_seed0": digest(synthetic_sepformer_state_dict(SepDims(), 0)),
        "sepformer_default_seed1": digest(synthetic_sepformer_state_dict(SepDims(), 1)),
        "sepformer_3spk_seed0": digest(synthetic_sepformer_state_dict(SepDims(n_spk=3), 0)),
        "dualpath_default_seed0": digest(synthetic_dualpath_state_dict(DualPathDims(), 0)),
        "dualpath_3spk_seed0_pos_enc_buffers": digest(synthetic_dualpath_state_dict(DualPathDims(n_spk=3), 0, pos_enc_buffers=True)),
    }
    assert got == want
