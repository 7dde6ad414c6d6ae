"""datasets_golden.json: the attributes of the reference's dataset classes that tests/test_datasets_host.py
compares centernet_amd/datasets.py with, recorded so that the test runs where the reference tree is absent.

    python tests/golden/gen_golden_datasets.py     # needs the reference tree
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    spec = importlib.util.spec_from_file_location("test_datasets_host",
                                                  os.path.join(os.path.dirname(HERE), "test_datasets_host.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    if not os.path.isdir(t.REF):
        raise SystemExit("reference tree not found at %s" % t.REF)
    out = {name: t.reference_attrs(name, file, cls) for name, file, cls in t.REF_CLASSES}
    with open(t.DATASETS_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", t.DATASETS_GOLDEN)


if __name__ == "__main__":
    main()
