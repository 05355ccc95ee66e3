"""examples/train_reference_shape.py is a training driver written in this repo that uses the `modules` boundary exactly the way the
reference's train.py does.  Two tests:

  * structural (CPU): both files are parsed and the ORDERED sequences of boundary calls -- name, number of positional arguments, keyword names, whether inside `torch.autocast` -- of the training
    iteration (train.py:168-201), of the optimizer / scaler / scheduler construction (:137-165) and of the evaluation loop (:237-262)
    are compared.  The example cannot drift away from the shape of train.py without this failing.  train.py's side is read from the
    reference checkout where it exists (and held to tests/golden/ref_driver_shape.json, oracle/gen_golden_checkout.py), from that
    file elsewhere;
  * executed (`-m gpu`; needs nothing but this repo): the example trains the procedural scene for 300 steps through render() + the
    compat FusedAdam + torch GradScaler and has to reach 20 dB on held-out views -- the drop-in loop runs on the driver's box, where
    the reference checkout (and with it tests/test_gpu_reference_train.py) is absent.
"""
import ast
import hashlib
import importlib.util
import json
import os

import pytest

from conftest import ROOT

REF = "/root/reference/train.py"
OURS = os.path.join(ROOT, "examples", "train_reference_shape.py")
DRIVER_SHAPE = os.path.join(ROOT, "tests", "golden", "ref_driver_shape.json")

# the calls that ARE the boundary + the optimisation protocol around it (attribute or plain name of the callee)
LOOP_CALLS = {"train", "update_density_grid", "get_rays", "render", "mse_loss", "distortion_loss", "mean", "zero_grad", "scale", "backward",
              "step", "update", "autocast"}
SETUP_CALLS = {"mark_invisible_cells", "GradScaler", "FusedAdam", "Adam", "CosineAnnealingLR", "parameters"}
EVAL_CALLS = {"eval", "no_grad", "autocast", "get_rays", "render"}
# constants the protocol hangs on
NEEDLES = ("warmup_steps = 256", "update_interval = 16", "exp_step_factor = 1 / 256 if hparams.scale > 0.5 else 0.0",
           "0.01 * MAX_SAMPLES / 3 ** 0.5", "step < warmup_steps", "step % update_interval == 0", "eps=1e-15", "hparams.lr / 30")


def _callee(node):
    f = node.func
    return f.attr if isinstance(f, ast.Attribute) else (f.id if isinstance(f, ast.Name) else None)


def _events(body, watch, in_autocast=False):
    """Calls to watched names in source (evaluation) order: (name, n positional, sorted keywords, inside torch.autocast?)."""
    out = []

    class V(ast.NodeVisitor):
        def __init__(self):
            self.auto = in_autocast

        def visit_With(self, node):
            is_auto = any(isinstance(i.context_expr, ast.Call) and _callee(i.context_expr) == "autocast" for i in node.items)
            for i in node.items:
                self.visit(i.context_expr)
            prev, self.auto = self.auto, self.auto or is_auto
            for st in node.body:
                self.visit(st)
            self.auto = prev

        def visit_Call(self, node):
            for a in list(node.args) + [k.value for k in node.keywords]:        # arguments are evaluated before the call
                self.visit(a)
            self.visit(node.func)
            name = _callee(node)
            if name in watch:
                out.append((name, len(node.args), tuple(sorted(k.arg for k in node.keywords if k.arg)), self.auto))

        def visit_If(self, node):
            # logging branches (`if step % 1000 == 0`) are not part of the protocol
            src = ast.unparse(node.test)
            if "% 1000" in src:
                return
            self.generic_visit(node)

    v = V()
    for st in body:
        v.visit(st)
    return out


def _main_parts(path):
    tree = ast.parse(open(path).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    loops = [n for n in ast.walk(main) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "step"]
    assert len(loops) == 1, "one `for step in range(...)` training loop expected in %s" % path
    train_loop = loops[0]
    evals = [n for n in ast.walk(main) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "test_step"]
    assert len(evals) == 1
    # the `with torch.no_grad():` block that holds the evaluation loop
    eval_with = next(n for n in ast.walk(main) if isinstance(n, ast.With) and any(e is evals[0] for e in ast.walk(n))
                     and any(isinstance(i.context_expr, ast.Call) and _callee(i.context_expr) == "no_grad" for i in n.items))
    setup = []
    for st in main.body:
        if st is train_loop or any(e is train_loop for e in ast.walk(st)):
            break
        setup.append(st)
    return main, setup, train_loop, eval_with


def driver_structure(path):
    """What the tests compare of a driver: the boundary-call sequences of its training iteration, setup and evaluation loop, its loop
    bounds and which of NEEDLES it contains (JSON-shaped)."""
    _, setup, loop, ev = _main_parts(path)
    src = ast.unparse(ast.parse(open(path).read()))
    d = {"loop": _events(loop.body, LOOP_CALLS), "setup": _events(setup, SETUP_CALLS), "eval": _events([ev], EVAL_CALLS),
         "loop_iter": ast.unparse(loop.iter), "needles": [n for n in NEEDLES if n in src]}
    return json.loads(json.dumps(d))


def line_similarity(ref_path, ours_path):
    """difflib ratio between the stripped non-empty lines of two files."""
    import difflib
    a = [x.strip() for x in open(ref_path).read().splitlines() if x.strip()]
    b = [x.strip() for x in open(ours_path).read().splitlines() if x.strip()]
    return difflib.SequenceMatcher(None, a, b).ratio()


def example_similarity(ref_path):
    """The example's line similarity with train.py, and the sha256 of the example file it was measured on."""
    return {"example_sha256": hashlib.sha256(open(OURS, "rb").read()).hexdigest(), "line_similarity": line_similarity(ref_path, OURS)}


def _reference_structure():
    stored = json.load(open(DRIVER_SHAPE))["train_py"]
    if os.path.exists(REF):
        assert driver_structure(REF) == stored
    return stored


def test_example_has_the_call_structure_of_train_py():
    ref, ours = _reference_structure(), driver_structure(OURS)
    # (1) the training iteration
    ev_r, ev_o = ref["loop"], ours["loop"]
    assert ev_r == ev_o, "training iteration differs:\n ref  %s\n ours %s" % (ev_r, ev_o)
    names = [e[0] for e in ev_r]
    assert names == ["train", "autocast", "update_density_grid", "get_rays", "render", "mse_loss", "distortion_loss", "mean", "zero_grad",
                     "scale", "backward", "step", "update", "step"], names                      # what the comparison is about
    assert [e[3] for e in ev_r] == [False, False] + [True] * 6 + [False] * 6                      # inside autocast: grid update .. loss
    # (2) optimizer / scaler / scheduler construction
    st_r, st_o = ref["setup"], ours["setup"]
    assert st_r == st_o, "setup differs:\n ref  %s\n ours %s" % (st_r, st_o)
    assert [e[0] for e in st_r] == ["mark_invisible_cells", "GradScaler", "parameters", "FusedAdam", "parameters", "Adam", "CosineAnnealingLR"]
    # (3) the evaluation loop
    ee_r, ee_o = ref["eval"], ours["eval"]
    assert ee_r == ee_o, "evaluation loop differs:\n ref  %s\n ours %s" % (ee_r, ee_o)
    assert ["render", 3, ["exp_step_factor", "test_time"], True] in ee_r
    # (4) the loop bounds and the constants the protocol hangs on
    src_r, src_o = ref["loop_iter"], ours["loop_iter"]
    assert src_r == src_o == "range(hparams.max_steps + 1)"
    assert ref["needles"] == ours["needles"] == list(NEEDLES)


def test_example_is_not_a_copy_of_train_py():
    """The example is written here: line-level similarity with the reference's driver stays far below what a copy would show.  Measured
    here where the checkout exists; elsewhere the ratio stored in tests/golden/ref_driver_shape.json is used, which holds for the
    example file whose sha256 it records (after a change to the example, oracle/gen_golden_checkout.py re-measures it)."""
    stored = json.load(open(DRIVER_SHAPE))["example_vs_train_py"]
    if os.path.exists(REF):
        now = example_similarity(REF)
        if now["example_sha256"] == stored["example_sha256"]:
            assert now == stored
        ratio = now["line_similarity"]
    else:
        assert hashlib.sha256(open(OURS, "rb").read()).hexdigest() == stored["example_sha256"], (
            "examples/train_reference_shape.py changed since its similarity with train.py was measured: run oracle/gen_golden_checkout.py "
            "where the reference checkout exists")
        ratio = stored["line_similarity"]
    assert ratio < 0.35


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--distortion_loss_w", "1e-3"), ("--half_opt",)], ids=["default", "distortion", "half_opt"])
def test_example_trains_the_procedural_scene(tmp_path, extra):
    spec = importlib.util.spec_from_file_location("train_reference_shape", OURS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--max_steps", "300", "--wh", "200", "--n_train", "12", "--n_test", "2", "--val_dir", str(tmp_path / "results"),
                    "--out", str(tmp_path / "run.json"), *extra])
    assert out["optimizer"].startswith("apex.optimizers.FusedAdam")            # train.py:143-149 finds `apex` (taichi-nerfs_amd/compat)
    assert out["log(elapsed_s,step,psnr,loss,rays,rm_s,vr_s)"][0][1] == 0
    assert os.path.exists(out["checkpoint"])
    assert out["test_psnr_avg"] > 20.0, out                                     # 300 steps on 12 views: it has to have learned the scene
