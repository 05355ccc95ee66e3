"""Drop-in checks.  Where the reference checkout exists: the reference's UNCHANGED train.py (and through it gui.py, datasets/,
opt.py) imports against this repo's `modules` package + the import-only stand-ins in taichi-nerfs_amd/compat/.  Everywhere: the
public callables have the reference's parameter names (read from the checkout where it exists and held to
tests/golden/ref_driver_shape.json, read from that file elsewhere)."""
import ast
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

REF = "/root/reference"
DRIVER_SHAPE = os.path.join(ROOT, "tests", "golden", "ref_driver_shape.json")
# (file under modules/, public callables) and (file, class whose __init__ parameters are compared)
FUNCTIONS = [("intersection.py", ["ray_aabb_intersection"]), ("ray_march.py", ["raymarching_train", "raymarching_test"]),
             ("volume_render_test.py", ["composite_test"]), ("rendering.py", ["render"]), ("distortion.py", ["distortion_loss"])]
CLASSES = [("networks.py", "NGP"), ("networks.py", "MLP"), ("hash_encoder.py", "HashEncoder"), ("hash_encoder_half.py", "HashEncoder")]


def reference_signatures(root):
    """Parameter names, in order, of the reference's public callables and class constructors under root/modules."""
    funcs, classes = {}, {}
    for fname, names in FUNCTIONS:
        sigs = {}
        for node in ast.walk(ast.parse(open(os.path.join(root, "modules", fname)).read())):
            if isinstance(node, ast.FunctionDef):
                sigs.setdefault(node.name, [a.arg for a in node.args.args])
        funcs[fname] = {n: sigs[n] for n in names}
    for fname, cname in CLASSES:
        tree = ast.parse(open(os.path.join(root, "modules", fname)).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name == cname:
                init = [f for f in node.body if isinstance(f, ast.FunctionDef) and f.name == "__init__"][0]
                classes["%s:%s" % (fname, cname)] = [a.arg for a in init.args.args]
    return {"functions": funcs, "classes": classes}


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "train.py")), reason="reference checkout not present")
def test_reference_train_py_imports_our_modules():
    code = (
        "import sys, warnings; warnings.filterwarnings('ignore');"
        "sys.path[:0]=[%r, %r, %r]; sys.argv=['train.py','--root_dir','x'];"
        "import importlib; m=importlib.import_module('train'); import modules;"
        "assert modules.__file__.startswith(%r), modules.__file__;"
        "names=[m.render.__module__, m.NGP.__module__, m.distortion_loss.__module__, m.save_deployment_model.__module__];"
        "assert names==['modules.rendering','modules.networks','modules.distortion','modules.utils'], names;"
        "import inspect; from modules.networks import NGP, MLP; from modules.hash_encoder import HashEncoder;"
        "print('ok')"
    ) % (os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "taichi-nerfs_amd", "compat"), REF,
         os.path.join(ROOT, "taichi-nerfs_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_public_signatures_match_reference():
    """Same parameter names (and order) for every public callable of the boundary."""
    import inspect
    stored = json.load(open(DRIVER_SHAPE))["signatures"]
    if os.path.exists(os.path.join(REF, "modules")):
        assert reference_signatures(REF) == stored
    import modules.intersection as mi, modules.ray_march as mr, modules.volume_render_test as mv, modules.rendering as rd
    import modules.networks as nw, modules.hash_encoder as he, modules.hash_encoder_half as hh, modules.distortion as ds
    mods = {"intersection.py": mi, "ray_march.py": mr, "volume_render_test.py": mv, "rendering.py": rd, "distortion.py": ds,
            "networks.py": nw, "hash_encoder.py": he, "hash_encoder_half.py": hh}
    for fname, names in FUNCTIONS:
        for n in names:
            assert list(inspect.signature(getattr(mods[fname], n)).parameters) == stored["functions"][fname][n], (fname, n)
    # class constructors
    for fname, cname in CLASSES:
        ours = inspect.signature(getattr(mods[fname], cname).__init__).parameters
        ref_args = stored["classes"]["%s:%s" % (fname, cname)]
        # every reference parameter, same order; extensions only as trailing keyword arguments with defaults
        assert list(ours)[:len(ref_args)] == ref_args, (fname, cname)
        assert all(ours[k].default is not inspect.Parameter.empty for k in list(ours)[len(ref_args):]), (fname, cname)
