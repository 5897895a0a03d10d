"""Writes tests/golden/reference_python_api.json: every use of the `ggnn` module that the
reference's Python examples (examples/python/*.py of the reference tree) make -- module
attributes, constructor / method / class-attribute calls and the keyword arguments they pass.

Names only, read syntactically with `ast`; no code of the examples is kept.  The fixture lets
tests/test_cabi.py::test_reference_python_examples_api_conformance check this package's surface
without the reference tree.  Regenerate deliberately with:
    python tests/golden/make_reference_python_api_golden.py <reference tree>"""
import ast
import glob
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_python_api.json")


def uses(source):
    """the `ggnn` uses of one example, in the order `ast.walk` visits them"""
    tree = ast.parse(source)
    instances = {}   # variable name -> attribute of ggnn it was constructed from
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call):
            f = node.value.func
            if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "ggnn":
                for t in node.targets:
                    if isinstance(t, ast.Name):
                        instances[t.id] = f.attr
    attributes, calls = [], []
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name):
            if node.value.id == "ggnn":
                attributes.append(node.attr)
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        call = None
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name):
            if f.value.id == "ggnn":
                call = {"kind": "module", "name": f.attr}
            elif f.value.id in instances:
                call = {"kind": "instance", "class": instances[f.value.id], "name": f.attr}
        elif (isinstance(f, ast.Attribute) and isinstance(f.value, ast.Attribute) and
              isinstance(f.value.value, ast.Name) and f.value.value.id == "ggnn"):
            call = {"kind": "class_attribute", "class": f.value.attr, "name": f.attr}
        if call is not None:
            call["keywords"] = [kw.arg for kw in node.keywords]
            calls.append(call)
    return {"module_attributes": attributes, "calls": calls}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    files = sorted(glob.glob(os.path.join(sys.argv[1], "examples", "python", "*.py")))
    if not files:
        raise SystemExit("no examples/python/*.py under " + sys.argv[1])
    out = [dict(file=os.path.relpath(p, sys.argv[1]), **uses(open(p).read())) for p in files]
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", OUT)
