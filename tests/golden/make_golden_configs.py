"""Golden settings for the config-file parser (authoring container only): the assignments of the reference's config/Latin_CTC.py,
config/Chinese.py and their `_base_` config/coco_transformer.py, each file executed on its own and its names stored as data.  The
test writes them back as plain assignment files and parses those with DTLRConfig.from_reference_file.

    python -m tests.golden.make_golden_configs REFERENCE_CHECKOUT     # writes tests/golden/g10_reference_configs.json
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ["coco_transformer.py", "Latin_CTC.py", "Chinese.py"]


def main(ref: str):
    files = {}
    for fn in FILES:
        ns: dict = {}
        p = os.path.join(ref, "config", fn)
        exec(compile(open(p).read(), p, "exec"), ns)     # noqa: S102 - plain assignment files
        files[fn] = {k: v for k, v in ns.items() if k != "__builtins__"}
    with open(os.path.join(HERE, "g10_reference_configs.json"), "w") as f:
        json.dump({"source": "reference config/ (one namespace per file, `_base_` kept)", "files": files}, f, indent=1, allow_nan=False)


if __name__ == "__main__":
    main(sys.argv[1])
