"""What the drivers share (ssl_mae_amd.driver): the config merge, the three synthetic clip sources'
draw orders, the labelled clip-set loader, and the rule that no driver imports another."""
import ast
import copy
import os

import pytest
import torch

from conftest import PKG

DRIVERS = ("run_dynamic", "run_privacy", "run_federated", "train_finetune", "temporal_ssl")
DEFAULTS = {"a": {"x": 1, "y": [1, 2]}, "b": {"z": None, "nested": {"p": 1, "q": 2}}}
T, S, NC, SEED = 3, 8, 5, 11
DS = {"dataset": {"clip_len": T, "image_size": S, "num_classes": NC}}


def _pixels(g, n):
    """The rule written out: pixels, then gain."""
    pixels = torch.rand(n, 3, T, S, S, generator=g)
    return (pixels - 0.45) / 0.226 * (0.3 + 1.4 * torch.rand(n, 1, T, 1, 1, generator=g))


# ------------------------------------------------------------------ merge
def test_merge_config_unknown_names_raise():
    from ssl_mae_amd.driver import merge_config
    with pytest.raises(ValueError, match=r"^\[ERROR\] Unknown config section: c$"):
        merge_config(DEFAULTS, {"c": {}})
    with pytest.raises(ValueError, match=r"^\[ERROR\] Unknown keys in a: \['v', 'w'\]$"):
        merge_config(DEFAULTS, {"a": {"w": 1, "x": 2, "v": 3}})
    with pytest.raises(ValueError, match=r"^\[ERROR\] Unknown keys in b\.nested: \['r'\]$"):
        merge_config(DEFAULTS, {"b": {"nested": {"r": 1}}})


def test_merge_config_values_and_none_sections():
    from ssl_mae_amd.driver import merge_config
    assert merge_config(DEFAULTS, None) == DEFAULTS and merge_config(DEFAULTS, {}) == DEFAULTS
    assert merge_config(DEFAULTS, {"a": None, "b": {"nested": None}}) == DEFAULTS
    got = merge_config(DEFAULTS, {"a": {"x": 7}, "b": {"z": "s", "nested": {"q": 9}}})
    assert got == {"a": {"x": 7, "y": [1, 2]}, "b": {"z": "s", "nested": {"p": 1, "q": 9}}}


def test_merge_config_shares_no_dict_with_the_defaults():
    from ssl_mae_amd.driver import merge_config
    before = copy.deepcopy(DEFAULTS)
    got = merge_config(DEFAULTS, {"b": {"nested": {"q": 9}}})
    got["a"]["x"] = 100
    got["b"]["nested"]["p"] = 100
    got["b"]["extra"] = 1
    assert DEFAULTS == before
    assert merge_config(DEFAULTS, {"b": {"nested": {"q": 9}}}) == {"a": before["a"],
                                                                  "b": {"z": None, "nested": {"p": 1, "q": 9}}}


def test_the_drivers_resolve_config_keeps_its_messages():
    from ssl_mae_amd import run_federated
    with pytest.raises(ValueError, match=r"^\[ERROR\] Unknown keys in federated\.non_iid: \['shards'\]$"):
        run_federated.resolve_config({"federated": {"non_iid": {"shards": 3}}})
    got = run_federated.resolve_config({"federated": {"non_iid": {"shards_per_client": 2}}})
    got["federated"]["non_iid"]["shards_per_client"] = 99
    assert run_federated.DEFAULTS["federated"]["non_iid"]["shards_per_client"] == 6


# ------------------------------------------------------------------ synthetic sources
def test_run_dynamic_source_draws_pixels_gain_labels_per_batch():
    from ssl_mae_amd.run_dynamic import SyntheticLoader
    cfg = dict(DS, runtime={"batch_size": 2, "num_warmup": 1, "num_measure": 1, "seed": SEED})
    loader = SyntheticLoader(cfg, "cpu")
    g = torch.Generator().manual_seed(SEED)
    want = []
    for _ in range(2):
        clip = _pixels(g, 2)
        want.append((clip, torch.randint(0, NC, (2,), generator=g)))
    got = list(loader)
    assert loader.batch_size == 2 and len(got) == 2 and got[0][0].shape == (2, 3, T, S, S)
    for (clip, label), (wclip, wlabel) in zip(got, want):
        assert torch.equal(clip, wclip) and torch.equal(label, wlabel)


def test_temporal_ssl_source_draws_pixels_gain_per_batch():
    from ssl_mae_amd.run_dynamic import SyntheticLoader
    from ssl_mae_amd.temporal_ssl import SyntheticClips
    clips = SyntheticClips(2, 2, T, S, "cpu", seed=SEED)
    g = torch.Generator().manual_seed(SEED)
    want = [_pixels(g, 2) for _ in range(2)]
    assert len(clips) == 2 and len(clips.batches) == 2
    for got, w in zip(clips, want):
        assert torch.equal(got, w)
    # equal seeds: the first batches agree, the second do not (run_dynamic's source drew labels in between)
    dyn = list(SyntheticLoader(dict(DS, runtime={"batch_size": 2, "num_warmup": 0, "num_measure": 2, "seed": SEED}),
                               "cpu"))
    assert torch.equal(dyn[0][0], want[0]) and not torch.equal(dyn[1][0], want[1])


def test_run_federated_source_draws_the_whole_set_at_once():
    from ssl_mae_amd.run_federated import SyntheticClips
    data = SyntheticClips(DS, 4, SEED, "cpu")
    g = torch.Generator().manual_seed(SEED)
    clips = _pixels(g, 4)
    labels = torch.randint(0, NC, (4,), generator=g)
    assert torch.equal(data.clips, clips) and torch.equal(data.labels, labels)
    assert data.items() == [(f"synthetic/{i}", int(y)) for i, y in enumerate(labels.tolist())]
    # neither of the per-batch sources' first batch
    g = torch.Generator().manual_seed(SEED)
    assert not torch.equal(data.clips[:2], _pixels(g, 2))


# ------------------------------------------------------------------ labelled loader
def _passes(loader, data, n=2):
    """The item indices of every batch of n passes (the clips identify their rows)."""
    out = []
    for _ in range(n):
        batches = []
        for clip, label in loader:
            idx = [next(i for i in range(len(data.clips)) if torch.equal(c, data.clips[i])) for c in clip]
            assert torch.equal(label, data.labels[idx])
            batches.append(idx)
        out.append(batches)
    return out


def test_labelled_loader_in_order_keeps_the_tail():
    from ssl_mae_amd.driver import SyntheticClips
    data = SyntheticClips(DS, 5, SEED, "cpu")
    loader = data.loader(data.items(), 2, False, 3)
    assert len(loader) == 3
    assert _passes(loader, data) == [[[0, 1], [2, 3], [4]]] * 2
    sub = data.loader(data.items()[3:] + data.items()[:1], 2, False, 3)      # a split file's subset, in its order
    assert _passes(sub, data, 1) == [[[3, 4], [0]]]


def test_labelled_loader_shuffle_drops_the_tail_and_reshuffles():
    from ssl_mae_amd.driver import SyntheticClips
    data = SyntheticClips(DS, 5, SEED, "cpu")
    first, second = _passes(data.loader(data.items(), 2, True, 3), data)
    for batches in (first, second):
        flat = [i for b in batches for i in b]
        assert [len(b) for b in batches] == [2, 2] and len(set(flat)) == 4 and set(flat) <= set(range(5))
    assert first != second
    assert len(data.loader(data.items(), 2, True, 3)) == 2
    # one seed, one sequence of passes: the written-out permutations
    g = torch.Generator().manual_seed(3)
    want = [torch.randperm(5, generator=g).tolist() for _ in range(2)]
    assert [[i for b in p for i in b] for p in (first, second)] == [w[:4] for w in want]
    assert _passes(data.loader(data.items(), 2, True, 3), data) == [first, second]


# ------------------------------------------------------------------ import graph
def _imported_modules(path):
    """Names of this package's modules that the file imports, function bodies included."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            found |= {a.name.split(".")[-1] for a in node.names if a.name.startswith("ssl_mae_amd")}
        elif isinstance(node, ast.ImportFrom) and (node.level > 0 or (node.module or "").startswith("ssl_mae_amd")):
            if node.module and node.module != "ssl_mae_amd":
                found.add(node.module.split(".")[-1])            # from .run_dynamic import x
            else:
                found |= {a.name for a in node.names}            # from . import run_dynamic
    return found


@pytest.mark.parametrize("name", DRIVERS)
def test_no_driver_imports_another(name):
    found = _imported_modules(os.path.join(PKG, "ssl_mae_amd", f"{name}.py"))
    assert found, "the walk found none of the package's imports"
    assert not found & (set(DRIVERS) | {"train_ssl"}) - {name}, sorted(found)


def test_train_ssl_stays_the_alias():
    from ssl_mae_amd import finetune, temporal_ssl, train_ssl
    assert train_ssl.main is temporal_ssl.main
    assert temporal_ssl.TopCEFn is finetune.TopCEFn
