"""Record tests/golden/conv_dispatch.json: the answers of ONE build of the library to the variant, statistics-tile and workspace
queries for every descriptor of tests/dispatch_cases.py.

    python tests/golden/make_dispatch_table.py <commit the library was built from> [path of that librho_hip.so]

The table pins the dispatch of the commit it was made from; it is not regenerated when the dispatch code is reorganised
(tests/test_conv_dispatch_host.py compares every later build with it).  Results only, in generator order, names interned.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

for k in [k for k in os.environ if k.startswith("RHO_")]:      # the library caches its knobs on first use
    del os.environ[k]

import dispatch_cases  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    table = dispatch_cases.run(sys.argv[2] if len(sys.argv) > 2 else None)
    table = {"built_from": sys.argv[1], **table}
    out = os.path.join(HERE, "conv_dispatch.json")
    with open(out, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(f"{out}: {len(table['rows'])} descriptors, {len(table['names'])} names, {os.path.getsize(out)} bytes")
