"""The host side of the ADD / ADD-S evaluation (no GPU): ``assign_errors`` and ``add_scores`` against a brute-force restatement on
hand-made and seeded groups (equal scores, more estimates than targets, a target without an estimate, an estimate in no group), the
AUC closed form against a numeric integration of the step curve, the recall decisions on inputs that keep every error farther from
its threshold than the derived float32 bound (asserted on the restatement first), ``evaluation.add_errors`` on host tensors against
``utils.metrics`` in float64, ``symmetry_residuals``, and tools/bop_eval.py with and without the new flags."""
import json
import math

import numpy as np
import pytest
import torch

from sam6d_amd import evaluation as ev
from sam6d_amd import groundtruth as gtm
from sam6d_amd.utils import metrics
from tests import add_ref as A
from tests import render_ref as R
from tests import test_gpu_add_eval as TA
from tests import test_host_bop_gt as TH


# ---------------------------------------------------------------------------------------------------------------- restatements
def brute_assign(pairs, scores, est_group, gt_group, n_targets):
    """{(e, g): error} -> per ground truth (error, estimate): the definition in plain loops."""
    error, taker = [math.inf] * len(gt_group), [-1] * len(gt_group)
    for grp, n in enumerate(n_targets):
        ests = sorted((e for e in range(len(est_group)) if est_group[e] == grp), key=lambda e: (-scores[e], e))[:n]
        taken = set()
        for e in ests:
            cands = [(pairs[(e, g)], g) for g in range(len(gt_group)) if gt_group[g] == grp and g not in taken and (e, g) in pairs]
            if cands:
                x, g = min(cands)
                taken.add(g)
                error[g], taker[g] = x, e
    return np.array(error), np.array(taker)


def brute_scores(error, threshold, auc_max):
    return (sum(e < t for e, t in zip(error, threshold)) / len(error), sum(max(0.0, 1.0 - e / auc_max) for e in error) / len(error))


def _pairs(est_group, gt_group, value):
    return {(e, g): value(e, g) for e in range(len(est_group)) for g in range(len(gt_group)) if est_group[e] == gt_group[g] and est_group[e] >= 0}


# ---------------------------------------------------------------------------------------------------------------- assignment
def test_assign_errors_on_hand_made_groups():
    """Group 0: two targets, four estimates, three of them with the same score (the two of lowest index are kept) and equal errors
    (the lower ground truth is taken); group 1: two targets, one estimate; group 2: a target without any estimate; estimate 5 is in
    no group."""
    est_group, gt_group, n_targets = [0, 0, 0, 0, 1, -1], [0, 0, 1, 1, 2], [2, 2, 1]
    scores = [0.9, 0.9, 0.5, 0.9, 0.3, 1.0]
    err = np.array([[4.0, 4.0, 9, 9, 9], [1.0, 2.0, 9, 9, 9], [0.1, 0.1, 9, 9, 9], [0.0, 0.0, 9, 9, 9], [9, 9, 7.0, 3.0, 9], [0, 0, 0, 0, 0.0]])
    got = ev.assign_errors(err, scores, est_group, gt_group, n_targets)
    # e0 (first of the equal scores) takes gt 0 (equal errors: the lower index), e1 the remaining gt 1; e3 and e2 are not kept
    assert got["estimate"].tolist() == [0, 1, -1, 4, -1] and got["error"].tolist() == [4.0, 2.0, math.inf, 3.0, math.inf]
    want = brute_assign(_pairs(est_group, gt_group, lambda e, g: float(err[e, g])), scores, est_group, gt_group, n_targets)
    assert np.array_equal(got["error"], want[0]) and np.array_equal(got["estimate"], want[1])
    # the triple form, with a pair across groups thrown in: it does not count
    pe, pg = np.nonzero(np.asarray(est_group)[:, None] == np.asarray(gt_group)[None, :])
    pe, pg = np.append(pe, 5), np.append(pg, 4)
    trip = ev.assign_errors((pe, pg, err[pe, pg]), scores, est_group, gt_group, n_targets)
    assert np.array_equal(trip["error"], got["error"]) and np.array_equal(trip["estimate"], got["estimate"])
    # no estimates at all; a NaN error counts as +inf
    none = ev.assign_errors(np.zeros((0, 5)), [], [], gt_group, n_targets)
    assert np.isposinf(none["error"]).all() and (none["estimate"] == -1).all()
    nan = ev.assign_errors(np.array([[np.nan, 5.0]]), [1.0], [0], [0, 0], [2])
    assert nan["error"].tolist() == [math.inf, 5.0] and nan["estimate"].tolist() == [-1, 0]


@pytest.mark.parametrize("seed", range(6))
def test_assign_errors_on_seeded_groups(seed):
    """Quantised scores and errors, so that ties of both kinds occur."""
    rs = np.random.RandomState(seed)
    groups = 4
    gt_group = rs.randint(0, groups, 9)
    n_targets = np.bincount(gt_group, minlength=groups)
    est_group = rs.randint(-1, groups, 14)
    scores = rs.randint(0, 4, 14) / 4.0
    err = rs.randint(0, 5, (14, 9)).astype(np.float64)
    got = ev.assign_errors(err, scores, est_group, gt_group, n_targets)
    want = brute_assign(_pairs(est_group, gt_group, lambda e, g: float(err[e, g])), scores.tolist(), est_group.tolist(), gt_group.tolist(), n_targets.tolist())
    assert np.array_equal(got["error"], want[0]) and np.array_equal(got["estimate"], want[1])
    assert (np.bincount(got["estimate"][got["estimate"] >= 0], minlength=14) <= 1).all()          # an estimate takes one target


def test_auc_closed_form_against_numeric_integration():
    """AUC(T) = mean_k max(0, 1 - e_k / T) is the area under t -> #{e_k < t} / K on [0, T] over T: a midpoint rule on M cells is off
    by at most one cell per step, K / M in all."""
    rs = np.random.RandomState(2)
    error = np.concatenate([rs.uniform(0, 150, 40), [0.0, 100.0, 99.999, math.inf, math.inf, 250.0]])
    T, M = 100.0, 400000
    mid = (np.arange(M) + 0.5) * (T / M)
    curve = np.searchsorted(np.sort(error), mid, side="left") / len(error)          # #{e_k < t} / K at the midpoints
    recall, auc = ev._recall_auc(error, np.full(len(error), 20.0), T)
    assert abs(auc - curve.mean()) <= len(error) / M
    assert recall == (error < 20.0).mean() and (recall, auc) == pytest.approx(brute_scores(error.tolist(), [20.0] * len(error), T), abs=1e-15)
    assert ev._recall_auc(np.zeros(0), np.zeros(0), T) == (0.0, 0.0)
    assert ev._recall_auc(np.array([0.0, math.inf]), np.array([1.0, 1.0]), T) == (0.5, 0.5)


# ---------------------------------------------------------------------------------------------------------------- the scores
def _score_case():
    """Two objects (a cube flagged symmetric through its symmetry set, a torus without one), seven targets in three images, ten
    estimates: some good, some poor, a group with more estimates than targets, a target without an estimate, an estimate whose
    (image, object) has no ground truth."""
    cube, torus = R.cube(40.0)[0], R.torus(8, 6)[0]
    models = {1: dict(vertices=cube, diameter=float(np.sqrt(19200.0)), symmetries=np.stack([np.eye(4), TA.RZ90])),
              2: dict(vertices=torus, diameter=170.0, info=dict(diameter=170.0))}
    gp = R.poses(7, seed=21).astype(np.float64)
    for g in range(7):
        gp[g, :3, 3] += (60.0 * g, -35.0 * g, 10.0 * g)
    gt = dict(im=np.array([0, 0, 0, 1, 1, 2, 2]), obj=np.array([1, 1, 2, 1, 2, 2, 2]), pose=gp)
    rs = np.random.RandomState(5)

    def near(g, angle, shift):
        P = gp[g].copy()
        P[:3, :3] = P[:3, :3] @ TA._rot(rs.standard_normal(3), angle)
        P[:3, 3] += shift
        return P
    spec = [(0, 1, near(0, 0.02, (1.0, 0.5, -2.0)), 0.9), (0, 1, near(1, 0.3, (9.0, -4.0, 6.0)), 0.9), (0, 1, near(1, 0.01, (0.5, 0.25, 0.5)), 0.4),
            (0, 2, near(2, 0.05, (2.0, 2.0, 2.0)), 0.7), (1, 1, near(3, 0.0, (0.0, 0.0, 0.0)) @ TA.RZ90, 0.8), (1, 2, near(4, 0.6, (20.0, 0.0, 0.0)), 0.6),
            (2, 2, near(5, 0.02, (0.0, 3.0, 0.0)), 0.5), (2, 1, near(5, 0.0, (0.0, 0.0, 0.0)), 1.0), (0, 2, near(2, 0.01, (0.5, 0.0, 0.0)), 0.7),
            (0, 2, near(2, 0.2, (30.0, 0.0, 0.0)), 0.95)]
    est = dict(im=np.array([s[0] for s in spec]), obj=np.array([s[1] for s in spec]), pose=np.stack([s[2] for s in spec]).astype(np.float32).astype(np.float64),
               score=np.array([s[3] for s in spec]))
    return models, est, gt


def test_add_scores_against_the_restatement():
    """Recall and AUC of the three rows from float64 pair errors, the brute-force assignment and the plain formulas.  The inputs keep
    every pair error farther from its recall threshold, and the errors an estimate chooses among farther from one another, than the
    derived float32 bound -- asserted on the restatement before the module is run -- so the decisions must agree; the AUC may differ
    by the mean bound over auc_max."""
    models, est, gt = _score_case()
    frac, T = 0.1, 100.0
    est_group, gt_group, keys = ev._group_ids(est, gt)
    assert est_group.tolist() == [0, 0, 0, 1, 2, 3, 4, -1, 1, 1] and len(keys) == 5
    n_targets = np.bincount(gt_group, minlength=len(keys)).tolist()
    value, bound = {}, 0.0
    for (e, g) in _pairs(est_group.tolist(), gt_group.tolist(), lambda e, g: 0.0):
        m = models[int(gt["obj"][g])]
        E, G = est["pose"][e:e + 1].astype(np.float32), gt["pose"][g:g + 1].astype(np.float32)
        r64 = A.errors(m["vertices"], E, G, np.float64)
        ba, bs = A.bounds(m["vertices"], E, G, r64)
        value[(e, g)] = dict(add=float(r64["add"][0]), adds=float(r64["adds"][0]), b=float(max(ba.mean(), bs.mean())) * (1 + 1e-9))
        bound = max(bound, value[(e, g)]["b"])
    sym = {1: True, 2: False}
    rows = dict(ADD=lambda p, g: p["add"], ADD_S=lambda p, g: p["adds"], ADD_or_S=lambda p, g: p["adds"] if sym[int(gt["obj"][g])] else p["add"])
    diam = np.array([models[int(o)]["diameter"] for o in gt["obj"]])
    for pick in rows.values():                                             # the condition on the inputs
        for (e, g), p in value.items():
            assert abs(pick(p, g) - frac * diam[g]) > p["b"]
            for (e2, g2), p2 in value.items():
                assert e2 != e or g2 == g or abs(pick(p, g) - pick(p2, g2)) > p["b"] + p2["b"]
    got = ev.add_scores(models, est, gt, frac=frac, auc_max=T, device="cpu")
    assert got["targets"] == 7 and got["estimates"] == 10 and got["frac"] == frac and got["auc_max"] == T
    for name, pick in rows.items():
        error, _ = brute_assign({k: pick(p, k[1]) for k, p in value.items()}, est["score"].tolist(), est_group.tolist(), gt_group.tolist(), n_targets)
        recall, auc = brute_scores(error.tolist(), (frac * diam).tolist(), T)
        assert got[name]["recall"] == pytest.approx(recall, abs=1e-15) and abs(got[name]["auc"] - auc) <= bound / T + 1e-15, (name, got[name], recall, auc)
    # what the case was built to show: the rotated cube is right under ADD-S only, one target has no estimate
    assert got["ADD_S"]["recall"] > got["ADD"]["recall"] and got["ADD_or_S"]["recall"] >= got["ADD"]["recall"]
    assert got["ADD"]["recall"] < 6 / 7 + 1e-12 and 0 < got["ADD"]["auc"] < 1
    flagged = {1: dict(models[1], symmetries=np.eye(4)[None], symmetric=True), 2: models[2]}
    assert ev.add_scores(flagged, est, gt, device="cpu") == got
    plain = {1: dict(models[1], symmetries=np.eye(4)[None]), 2: models[2]}
    assert ev.add_scores(plain, est, gt, device="cpu")["ADD_or_S"] == got["ADD"]
    empty = ev.add_scores(models, dict(im=np.zeros(0, int), obj=np.zeros(0, int), pose=np.zeros((0, 4, 4)), score=np.zeros(0)), gt, device="cpu")
    assert empty["ADD"] == dict(recall=0.0, auc=0.0) and empty["targets"] == 7 and empty["estimates"] == 0


# ---------------------------------------------------------------------------------------------------------------- the errors
@pytest.mark.parametrize("V", [1, 8, 48, 64])
def test_add_errors_on_host_tensors_against_utils_metrics(V):
    """float64 host inputs (rounded to float32 by the module, as every operand is) against utils.metrics in float64 on the same
    float32 values: each mean within the mean of the derived per-vertex bounds; equal to the numpy restatement bit for bit."""
    v = R.cube(40.0)[0] if V == 8 else TA.mesh(V)
    est, gt = TA.pose_pairs(3, seed=V)
    got = ev.add_errors(torch.from_numpy(v).double(), torch.from_numpy(est).double(), torch.from_numpy(gt).double(), per_vertex=True)
    assert got["add"].dtype == torch.float64 and not got["add"].is_cuda and got["adds_per_vertex"].shape == (3, V)
    r32, r64 = A.errors(v, est, gt, np.float32), A.errors(v, est, gt, np.float64)
    assert TA.same({k: x.numpy() for k, x in got.items()}, r32)
    ba, bs = A.bounds(v, est, gt, r64)
    e64, g64, v64 = torch.from_numpy(est).double(), torch.from_numpy(gt).double(), torch.from_numpy(v).double()
    add = metrics.add_error(e64[:, :3, :3], e64[:, :3, 3], g64[:, :3, :3], g64[:, :3, 3], v64).numpy()
    adds = metrics.adds_error(e64[:, :3, :3], e64[:, :3, 3], g64[:, :3, :3], g64[:, :3, 3], v64).numpy()
    assert (np.abs(got["add"].numpy() - add) <= ba.mean(1) * (1 + 1e-9)).all() and (np.abs(got["adds"].numpy() - adds) <= bs.mean(1) * (1 + 1e-9)).all()
    assert (add > 1).all() and (adds > 0.5).all() or V == 1
    with pytest.raises(ValueError, match="vertex"):
        ev.add_errors(np.zeros((0, 3)), est, gt)
    with pytest.raises(ValueError, match="shape"):
        ev.add_errors(v, est, gt[:2])
    none = ev.add_errors(v, est[:0], gt[:0], per_vertex=True, which=("adds",))
    assert none["adds"].shape == (0,) and none["adds_per_vertex"].shape == (0, V) and none["add"] is None


def test_symmetry_residuals_on_the_host():
    cube = R.cube(40.0)[0]
    info = dict(symmetries_discrete=[TA.RZ90.reshape(-1).tolist()])
    syms = ev.symmetry_transforms(info)
    r = ev.symmetry_residuals(cube, syms, diameter=float(np.sqrt(19200.0)), device="cpu")
    assert r["mean"].tolist() == [0.0, 0.0] and r["max"].tolist() == [0.0, 0.0] and r["max_fraction"].tolist() == [0.0, 0.0]
    off = np.eye(4)
    off[:3, :3] = TA._rot((0, 0, 1), np.pi / 4)
    r = ev.symmetry_residuals(cube, off[None], device="cpu")
    want = math.hypot(40.0, 40.0 * math.sqrt(2) - 40.0)                    # (40, 40) turns to (0, 56.57): the nearest corner
    assert abs(r["mean"][0] - want) < 1e-4 and abs(r["max"][0] - want) < 1e-4 and "max_fraction" not in r


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_bop_eval_tool_with_and_without_the_new_flags(tmp_path, capsys):
    """Without --add / --check-symmetries the printed keys are the ones of before; --add adds the ``add`` block = add_scores on the
    loaded dataset, --check-symmetries the ``symmetries`` block and a warning for the set that does not fit its mesh."""
    bop_eval = TH._tools()[1]
    root = tmp_path / "ds"
    models, gt, images, scene = TH._write_dataset(root)
    images["depth"] = (np.rint(images["depth"] * 10).astype(np.uint16).astype(np.float32) * np.float32(0.1))
    TH._result_files(tmp_path, gt, gtm.instance_ground_truth(models, gt, images, device="cpu"))
    info = {str(obj): gtm.model_info(models[obj]["vertices"], device="cpu") for obj in (1, 2)}
    info["1"]["symmetries_discrete"] = [TA.RZ90.reshape(-1).tolist()]
    bad = np.eye(4)
    bad[:3, :3] = TA._rot((0, 0, 1), 0.35)                                 # the torus has eight segments: 45 degrees would fit
    info["2"]["symmetries_discrete"] = [bad.reshape(-1).tolist()]
    (root / "models_eval" / "models_info.json").write_text(json.dumps(info))
    args = ["--results", str(tmp_path / "poses.csv"), "--dataset", str(root), "--device", "cpu"]
    before = ["AR", "AR_MSPD", "AR_MSSD", "AR_VSD", "dropped_estimates", "estimates", "images", "recalls_MSPD", "recalls_MSSD", "recalls_VSD",
              "results", "seconds", "targets", "unrenderable"]
    plain = bop_eval.main(args)
    line = capsys.readouterr()
    assert sorted(plain) == before and list(json.loads(line.out)) == list(plain) and line.err == ""
    both = bop_eval.main(args + ["--add", "--check-symmetries", "--auc-max", "50"])
    line = capsys.readouterr()
    assert sorted(both) == sorted(before + ["add", "symmetries"]) and json.loads(line.out) == both
    assert TH._line({k: v for k, v in both.items() if k not in ("add", "symmetries")}) == TH._line(plain)
    assert list(both)[:len(plain) - 4] == list(plain)[:len(plain) - 4]     # the new blocks stand after the scores, before the bookkeeping
    add = both["add"]
    assert sorted(add) == ["ADD", "ADD_S", "ADD_or_S", "auc_max", "estimates", "frac", "targets"] and add["targets"] == 6 and add["auc_max"] == 50.0
    lm, lg, _, index = bop_eval.load_dataset(str(root), "test", {TH.SCENE})
    res = ev.read_bop_csv(tmp_path / "poses.csv")
    pose = np.tile(np.eye(4), (len(res["im"]), 1, 1))
    pose[:, :3, :3], pose[:, :3, 3] = res["R"], res["t"]
    est = dict(im=np.array([index[(int(s), int(i))] for s, i in zip(res["scene"], res["im"])]), obj=res["obj"], score=res["score"], pose=pose)
    assert ev.add_scores(lm, est, lg, frac=0.1, auc_max=50.0, device="cpu") == add
    assert add["ADD_S"]["recall"] >= add["ADD"]["recall"] > 0 and 0 < add["ADD"]["auc"] < 1          # a few units off
    sym = both["symmetries"]
    assert sym["1"]["ok"] and sym["1"]["max_fraction"] == 0.0 and sym["1"]["transforms"] == 2
    assert not sym["2"]["ok"] and sym["2"]["worst"] == 1 and sym["2"]["max_fraction"] > 0.01
    assert "object 2" in line.err and "object 1" not in line.err
