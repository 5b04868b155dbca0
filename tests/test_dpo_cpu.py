"""CPU-only checks of the Diffusion-DPO boundary (`pipeline/dpo.py`): include/ddpo_dpo.h against lib_dpo._SIGS and the library's exports
(its own ABI version, nothing of it in ddpo_hip.h), the entry's argument validation (which returns before any launch), the closed form of
the error difference and of the gradient against float64 autograd of the authors' form (tests/_dpo_oracle.py), and the host side: the
pairing, its shards, the loader, the config and the argument check.  No device compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ddpo_amd import lib as L

import _dpo_oracle as DO
from _abi_check import check_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ddpo_dpo.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_signatures_match_the_header_prototypes():
    """tests/test_abi_cpu.py::test_signatures_match_the_header_prototypes, applied to include/ddpo_dpo.h and lib_dpo._SIGS."""
    from ddpo_amd import lib_dpo as LD
    check_signatures(HDR, LD._SIGS, 2, returns=("int",))


def test_library_exports_every_declared_symbol_under_its_own_version():
    from ddpo_amd import lib_dpo as LD
    declared = set(re.findall(r"\b(ddpo_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(LD.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ddpo_dpo.h but not exported"
    assert LD.load().ddpo_dpo_abi_version() == LD.ABI_VERSION == 1
    # versioned on its own: ddpo_hip.h, lib.ABI_VERSION and lib._SIGS know nothing of it
    main = open(os.path.join(ROOT, "include", "ddpo_hip.h")).read()
    for name in LD.EXPORTED_SYMBOLS:
        assert name not in main and name not in L._SIGS


def test_binding_refuses_a_version_mismatch(monkeypatch):
    from ddpo_amd import lib_dpo as LD
    monkeypatch.setattr(LD, "_lib", None)
    monkeypatch.setattr(LD, "ABI_VERSION", 2)
    with pytest.raises(L.DdpoHipError, match="Diffusion-DPO ABI version 1.*expects 2"):
        LD.load()
    assert LD._lib is None


def test_entry_rejects_bad_arguments_before_any_launch():
    """Every DDPO_EINVAL case of include/ddpo_dpo.h on host buffers: the checks come before the first launch, so no device is touched."""
    from ddpo_amd import lib_dpo as LD
    fn = LD.load().ddpo_dpo_pair_fwd_bwd
    B, chw = 4, 8
    bufs = [np.zeros(B * chw + 4, dtype=np.float32) for _ in range(7)]
    a16 = lambda a: a.ctypes.data + (-a.ctypes.data % 16)                  # 16-byte aligned address inside the buffer
    ec, eu, rc, ru, tg, dc, du = (ctypes.c_void_p(a16(a)) for a in bufs)
    pref = np.asarray([1, -1, -1, 1], dtype=np.float32)
    small = [np.zeros(B * 2, dtype=np.float32), np.zeros(B // 2 * 3, dtype=np.float32), np.zeros(5, dtype=np.float32)]
    pr, pp, inf = (ctypes.c_void_p(a.ctypes.data) for a in small)
    prp = ctypes.c_void_p(pref.ctypes.data)

    def call(ec=ec, eu=eu, rc=rc, ru=ru, tg=tg, pref=prp, beta=5000.0, cfg=1, dc=dc, du=du, pr=pr, pp=pp, inf=inf, B=B, chw=chw):
        return fn(ec, eu, rc, ru, tg, pref, 5.0, beta, cfg, dc, du, pr, pp, inf, B, chw, None)

    null = ctypes.c_void_p(0)
    off = lambda p: ctypes.c_void_p(p.value + 4)
    cases = [dict(ec=null), dict(rc=null), dict(tg=null), dict(pref=null), dict(dc=null), dict(pr=null), dict(pp=null), dict(inf=null),
             dict(eu=null), dict(ru=null), dict(du=null),                              # required under train_cfg
             dict(cfg=0, ec=null), dict(cfg=0, rc=null), dict(cfg=0, dc=null),
             dict(B=0), dict(B=-4), dict(B=3), dict(B=1),
             dict(chw=0), dict(chw=-4), dict(chw=6),
             dict(beta=0.0), dict(beta=-0.1), dict(beta=float("nan")), dict(beta=float("inf")),
             dict(ec=off(ec)), dict(rc=off(rc)), dict(tg=off(tg)), dict(dc=off(dc)),      # float4 access: 16-byte alignment
             dict(eu=off(eu)), dict(ru=off(ru)), dict(du=off(du)),
             dict(cfg=0, ec=off(ec)), dict(cfg=0, tg=off(tg))]
    for kw in cases:
        assert call(**kw) == -1, kw
    for a in bufs + small:
        assert not a.any()


# ------------------------------------------------------------------------------------------------ the closed form against float64 autograd
def _case(train_cfg, B=6, chw=4100, seed=0):
    g = torch.Generator().manual_seed(seed + int(train_cfg))
    shp = (B, 4, chw // 4, 1)
    ec, eu, tg = (torch.randn(shp, generator=g, dtype=torch.float64) for _ in range(3))
    rc = ec + 1e-2 * torch.randn(shp, generator=g, dtype=torch.float64)
    ru = eu + 1e-2 * torch.randn(shp, generator=g, dtype=torch.float64)
    pref = np.asarray([1, -1, -1, 1, 0, 0], dtype=np.float32)[:B]          # one pair of each label
    return ec, (eu if train_cfg else None), rc, (ru if train_cfg else None), tg, pref


@pytest.mark.parametrize("train_cfg", [True, False])
def test_closed_form_equals_float64_autograd_of_the_authors_form(train_cfg):
    ec, eu, rc, ru, tg, pref = _case(train_cfg)
    B, chw, n = 6, 4100, 3
    with torch.no_grad():                 # beta on the host, so that the larger |s_p| is 2: the sigmoid is off its centre and q enters the gradient
        _, _, _, D0, _, _ = DO.loss_and_info_torch(ec, eu, rc, ru, tg, pref, 5.0, 1.0, train_cfg)
    beta = 2.0 / float((0.5 * (D0[0:4:2] - D0[1:4:2])).abs().max())
    tec = ec.clone().requires_grad_(True)
    teu = eu.clone().requires_grad_(True) if train_cfg else None
    loss, info, m, D, s, loss_p = DO.loss_and_info_torch(tec, teu, rc, ru, tg, pref, 5.0, beta, train_cfg)
    loss.backward()
    assert float(loss_p[2].detach()) == 0.0 and float(s[2].detach()) == 0.0      # the tie
    assert float(s.detach().abs().max()) == pytest.approx(2.0)
    # the same numbers from the closed form, evaluated in float64
    e = DO.guided(ec, eu, 5.0, train_cfg)
    delta = DO.guided(ec - rc, None if eu is None else eu - ru, 5.0, train_cfg)
    a = tg - e
    D_cf = -(2 * (a * delta).flatten(1).sum(1) + (delta ** 2).flatten(1).sum(1)) / chw
    # the difference of two mean squared errors cancels |m| ~ 27 (g = 5) or ~ 2 against |D| ~ 1e-3 in float64
    assert float((D_cf - D.detach()).abs().max()) < 1e-13
    y = torch.from_numpy((pref[0::2] - pref[1::2]) / 2).double()
    s_cf = -0.5 * beta * y * (D_cf[0::2] - D_cf[1::2])
    q = torch.sigmoid(-s_cf)
    c_even = (0.5 * beta * y * q / n) * (-2.0 / chw)
    de = torch.stack([c_even, -c_even], 1).reshape(B, 1, 1, 1) * a
    gc = 5.0 * de if train_cfg else de
    gmax = float(tec.grad.abs().max())
    assert float((gc - tec.grad).abs().max()) < 1e-10 * gmax
    assert float(tec.grad[4:].abs().max()) == 0.0 and float(tec.grad[:4].abs().min()) > 0.0
    if train_cfg:
        assert float(((1 - 5.0) * de - teu.grad).abs().max()) < 1e-10 * float(teu.grad.abs().max())
    # and the fp32 restatement of the HIP pass says the same to fp32 accuracy
    f = lambda t: None if t is None else t.numpy().astype(np.float32)
    t64 = lambda v: None if v is None else torch.from_numpy(v).double()
    m32, D32, s32, lp32, q32, info32, dc32, du32 = DO.closed_form_numpy(f(ec), f(eu), f(rc), f(ru), f(tg), pref, 5.0, beta, train_cfg)
    tec2 = t64(f(ec)).requires_grad_(True)
    teu2 = t64(f(eu)).requires_grad_(True) if train_cfg else None
    loss2, info2, m2, D2, s2, lp2 = DO.loss_and_info_torch(tec2, teu2, t64(f(rc)), t64(f(ru)), t64(f(tg)), pref, 5.0, beta, train_cfg)
    loss2.backward()
    Dmax = float(D2.detach().abs().max())
    assert float(np.abs(D32 - D2.detach().numpy()).max()) < 2e-5 * Dmax
    assert float(np.abs(m32 - m2.detach().numpy()).max()) < 2e-6 * float(m2.detach().max())
    assert float(np.abs(s32 - s2.detach().numpy()).max()) < 2e-5 * 2.0
    assert float(np.abs(lp32 - lp2.detach().numpy()).max()) < 2e-5 * float(lp2.detach().max())
    assert info32.shape == (5,) and info32[1] == np.float32(float(info2["implicit_acc"].detach()))
    for i, k in enumerate(DO.INFO_KEYS):
        want = float(info2[k].detach())
        if k != "implicit_acc":
            assert abs(float(info32[i]) - want) < 2e-5 * max(abs(want), Dmax), k
    assert float(np.abs(dc32 - tec2.grad.numpy()).max() / tec2.grad.abs().max()) < 5e-5
    if train_cfg:
        assert float(np.abs(du32 - teu2.grad.numpy()).max() / teu2.grad.abs().max()) < 5e-5


def test_error_difference_is_exactly_zero_where_the_networks_agree():
    ec, eu, rc, ru, tg, pref = _case(True)
    _, info, _, D, s, loss_p = DO.loss_and_info_torch(ec, eu, ec, eu, tg, pref, 5.0, 5000.0, True)
    assert float(D.abs().max()) == 0.0 and float(info["margin"]) == 0.0
    assert float(loss_p[0]) == pytest.approx(np.log(2.0), rel=1e-15) and float(loss_p[2]) == 0.0
    f = lambda t: t.numpy().astype(np.float32)
    m32, D32, s32, lp32, q32, info32, dc32, _ = DO.closed_form_numpy(f(ec), f(eu), f(ec), f(eu), f(tg), pref, 5.0, 5000.0, True)
    assert (D32 == 0.0).all() and (s32 == 0.0).all() and info32[2] == 0.0 and (q32 == 0.5).all()
    assert lp32[0] == lp32[1] == np.log1p(np.float32(1.0)) and lp32[2] == 0.0
    assert info32[0] == np.float32((lp32[0] + lp32[1] + lp32[2]) / np.float32(3))     # ties count in n
    assert np.abs(dc32[:4]).min() > 0 and np.isfinite(dc32).all() and not dc32[4:].any()


# ------------------------------------------------------------------------------------------------ pairs on the host
def _store(seed=0):
    """40 rows over 5 prompts with 12, 9, 1, 8, 10 rows; rewards on a grid of 4 values, so ties occur."""
    rs = np.random.RandomState(seed)
    prompts = np.repeat(np.asarray(["heron", "ant", "yak", "cat", "bee"]), [12, 9, 1, 8, 10])
    perm = rs.permutation(len(prompts))
    return prompts[perm], rs.randint(0, 4, len(prompts)).astype(np.float64) * 0.25


def test_make_pairs():
    from ddpo_amd.utils.bucket import make_pairs, pair_counts, shard_pairs
    prompts, rewards = _store()
    idx, y = make_pairs(prompts, rewards, 3)
    assert idx.dtype == np.int64 and idx.ndim == 2 and idx.shape[1] == 2 and y.dtype == np.float32 and y.shape == (len(idx),)
    assert len(np.unique(idx)) == idx.size                                             # every index at most once
    assert (prompts[idx[:, 0]] == prompts[idx[:, 1]]).all()                            # both rows of a pair share the prompt
    assert np.array_equal(y, np.sign(rewards[idx[:, 0]] - rewards[idx[:, 1]]).astype(np.float32)) and (y != 0).all()
    assert (y > 0).any() and (y < 0).any()
    # ties and leftovers dropped: the pairs formed before ties leave are sum_k floor(n_k / 2); the ties are those of THIS pairing
    formed = 6 + 4 + 0 + 4 + 5
    ties, leftover = pair_counts(prompts, len(idx))
    assert leftover == 40 - 2 * formed == 2 and ties == formed - len(idx) and 0 < ties < formed
    rs = np.random.RandomState(3)                                                      # the documented draws, replayed
    mine = np.concatenate([rs.permutation(np.flatnonzero(prompts == p))[:2 * (int((prompts == p).sum()) // 2)].reshape(-1, 2)
                           for p in np.unique(prompts)])
    assert len(mine) == formed and int((rewards[mine[:, 0]] == rewards[mine[:, 1]]).sum()) == ties
    kept = mine[rewards[mine[:, 0]] != rewards[mine[:, 1]]]
    assert np.array_equal(idx, kept[rs.permutation(len(kept))])
    # the same seed gives the same pairs, another seed others
    idx2, y2 = make_pairs(prompts, rewards, 3)
    assert np.array_equal(idx, idx2) and np.array_equal(y, y2)
    idx3, _ = make_pairs(prompts, rewards, 4)
    assert idx3.shape != idx.shape or not np.array_equal(idx, idx3)
    # shards of 2 hosts: disjoint whole pairs, P // 2 each, of the one pairing
    a, ya = shard_pairs(idx, y, 0, 2)
    b, yb = shard_pairs(idx, y, 1, 2)
    assert len(a) == len(b) == len(idx) // 2 and not set(a.reshape(-1)) & set(b.reshape(-1))
    assert np.array_equal(np.concatenate([a, b]), idx[:2 * (len(idx) // 2)]) and np.array_equal(np.concatenate([ya, yb]), y[:2 * (len(idx) // 2)])
    # no prompt occurs twice / every pair is a tie
    with pytest.raises(ValueError, match="no prompt occurs twice.*--identical_batch True"):
        make_pairs(np.asarray(["a", "b", "c"]), np.asarray([1.0, 2.0, 3.0]), 0)
    with pytest.raises(ValueError, match="--identical_batch True"):
        make_pairs(np.asarray(["a", "a"]), np.asarray([1.0, 1.0]), 0)


class _Reader:
    """What PairLoader touches of bucket.LocalReader."""

    def __init__(self, prompts, rewards):
        self.rows = [{"inference_prompts": p, "training_prompts": np.asarray([p + " one", p + " two", p + " three"]), "jpeg": np.float32(r),
                      "vae": np.full((2, 2, 8), i, dtype=np.float32)} for i, (p, r) in enumerate(zip(prompts, rewards))]

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.rows[i]

    def get(self, sl, field):
        return np.stack([np.asarray(r[field]) for r in self.rows[sl]])


class _Tok:
    model_max_length = 4

    def __call__(self, texts, **kw):
        self.seen = list(texts)
        return type("T", (), {"input_ids": np.asarray([[len(t)] * 4 for t in texts])})()


def test_pair_loader_batches_shards_and_labels():
    from ddpo_amd.utils.bucket import PairLoader, make_pairs
    prompts, rewards = _store()
    idx, y = make_pairs(prompts, rewards, 7)
    seen = []
    for host in range(2):
        tok = _Tok()
        ld = PairLoader(_Reader(prompts, rewards), tok, 4, "jpeg", host_id=host, n_hosts=2)
        kept, ties, leftover = ld.pair(7)
        assert kept == len(idx) and leftover == 2 and kept + ties == 19
        mine = len(idx) // 2
        assert len(ld) == mine // 2                                                  # drop-last over this host's whole pairs
        batches = list(ld)
        assert len(batches) == len(ld)
        for b, batch in enumerate(batches):
            rows = batch["shuffled_idxs"]
            want = idx[host * mine + 2 * b:host * mine + 2 * b + 2]
            assert np.array_equal(rows.reshape(2, 2), want)                            # pairs on adjacent rows, in the pairing's order
            yy = y[host * mine + 2 * b:host * mine + 2 * b + 2]
            assert batch["pref"].dtype == np.float32 and batch["pref"].tolist() == [yy[0], -yy[0], yy[1], -yy[1]]
            assert np.array_equal(batch["vae"][:, 0, 0, 0], rows.astype(np.float32)) and batch["vae"].shape == (4, 2, 2, 8)
            assert np.array_equal(batch["input_ids"][0], batch["input_ids"][1]) and np.array_equal(batch["input_ids"][2], batch["input_ids"][3])
            seen += rows.tolist()
    assert len(set(seen)) == len(seen)
    with pytest.raises(ValueError, match="even"):
        PairLoader(_Reader(prompts, rewards), _Tok(), 3, "jpeg")
    # max_train_samples: only the first rows are paired
    ld = PairLoader(_Reader(prompts, rewards), _Tok(), 2, "jpeg", max_train_samples=20)
    ld.pair(0)
    assert ld.n_rows == 20 and int(ld.idx.max()) < 20


# ------------------------------------------------------------------------------------------------ config, flags
def test_config_defaults_parser_and_argument_check(tmp_path, monkeypatch):
    import inspect
    import config.base as C
    from ddpo_amd.training.diffusion_dpo import check_dpo_args
    from pipeline import dpo
    monkeypatch.chdir(tmp_path)
    d = C.base["dpo"]
    assert d["dpo_beta"] == 5000.0 and d["pair_seed"] == 0
    assert set(d) == (set(C.base["train"]) - {"weighted_batch", "weighted_dataset", "per_prompt_weights"}) | {"dpo_beta", "pair_seed"}
    assert all(d[k] == C.base["train"][k] for k in d if k in C.base["train"])
    # the other experiments know nothing of it, and `train` is what it was
    for exp in ("train", "sample", "pg"):
        assert "dpo_beta" not in C.base[exp] and "pair_seed" not in C.base[exp]
    assert C.base["train"] == dict(C._TRAIN_DEFAULTS) and len(C.base["train"]) == 28 and C.base["train"]["weighted_batch"] is False
    for name in ("compressed_animals_dpo", "a_animals_dpo"):
        ds = getattr(C, name)
        assert ds["sample"] == C._SAMPLE_ALL and "train" not in ds and ds["dpo"]["train_batch_size"] % 2 == 0 and ds["pg"] == {}
    assert C.compressed_animals_rwr["sample"] == C._SAMPLE_ALL and "dpo" not in C.compressed_animals_rwr
    common = ["--dataset", "compressed-animals-dpo", "--logbase", str(tmp_path / "run")]
    a0 = dpo.Parser(common).parse_args("dpo", process_index=3)
    assert a0.dpo_beta == 5000.0 and a0.pair_seed == 0 and a0.seed == 3 and a0.filter_field == "jpeg" and a0.train_cfg is True
    assert a0.savepath.endswith("models/1") and a0.loadpath.endswith("samples/0")
    a1 = dpo.Parser(common + ["--dpo_beta", "2500", "--pair_seed", "5"]).parse_args("dpo")
    assert a1.dpo_beta == 2500.0 and isinstance(a1.dpo_beta, float) and a1.pair_seed == 5 and isinstance(a1.pair_seed, int)
    assert check_dpo_args(a1.dpo_beta, a1.train_batch_size) is None
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "finite number > 0" in check_dpo_args(bad, 2)
    assert "train_batch_size must be even" in check_dpo_args(5000.0, 3)
    src = inspect.getsource(dpo.main)
    assert 0 < src.index("check_dpo_args(") < src.index("load(None)")                 # before any model is loaded
    assert src.index("KLReference(") < src.index("load(modelpath)")                    # the reference is the pretrained model
    assert "reject_lora_flags" in src and 'parse_args("dpo", process_index=worker_id)' in src


def test_other_entry_points_never_import_the_binding():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import pipeline.finetune, pipeline.policy_gradient; "
            "assert 'ddpo_amd.lib_dpo' not in sys.modules and 'ddpo_amd.training.diffusion_dpo' not in sys.modules" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
