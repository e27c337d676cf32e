"""CPU: the host-side dispatch of the convolution and weight-gradient entry points, pinned descriptor by descriptor.

tests/golden/conv_dispatch.json holds what rho_conv_variant, rho_conv_stats_tiles, rho_conv_workspace_bytes and
rho_conv_wgrad_variant answered for every descriptor of tests/dispatch_cases.py in the build of the commit named in the file
("built_from").  The queries need no GPU, so the library under test is asked the same questions here and must give the same
answers: the kernel a descriptor gets, its statistics rows and its workspace are part of the contract with the engine, which
sizes buffers from the queries and launches afterwards."""
import json
import os
import subprocess
import sys

import pytest

import dispatch_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "conv_dispatch.json")


@pytest.fixture(scope="module")
def golden():
    with open(TABLE) as f:
        return json.load(f)


def test_table_matches_the_generator(golden):
    n = len(DC.cases())
    assert 2000 <= n <= 5000
    assert len(golden["rows"]) == n
    assert os.path.getsize(TABLE) < 256 * 1024
    assert golden["built_from"]


def test_generator_reaches_what_it_must(golden):
    """Conditions on the generator, judged on the recorded answers."""
    import test_gpu_exact_backward as TB
    import test_gpu_exact_conv as TF
    names, rows = golden["names"], golden["rows"]
    fwd = {names[r[1]] for r in rows if r[0] == 0}
    wg = {names[r[i + 1]] for r in rows for i in (4, 6) if r[i] == 0}
    pinned = set(TF.EXPECT.values()) | TF.PHASE_VARIANTS
    assert not pinned - fwd, sorted(pinned - fwd)
    pinned_w = set(TB.EXPECT_W.values()) | TB.PHASE_W
    assert not pinned_w - wg, sorted(pinned_w - wg)
    rcs = {r[0] for r in rows}
    assert {DC.E_ARG, DC.E_ALIGN, DC.E_SHAPE, 0} <= rcs, rcs
    assert sum(1 for r in rows if r[3] > 0) >= 5                       # workspace wanted
    assert any(r[2] > 0 for r in rows) and any(r[2] == 0 and r[0] == 0 for r in rows)
    # stage ordering: a statistics-tile or workspace query that succeeds for a descriptor whose launch is refused
    assert sum(1 for r in rows if r[0] != 0 and (r[2] > 0 or r[3] > 0)) >= 10


def test_library_answers_as_recorded(golden):
    """A fresh process without any RHO_* variable (the library caches its knobs in statics on first use)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RHO_")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "dispatch_cases.py")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    cases = DC.cases()
    assert len(got["rows"]) == len(golden["rows"]) == len(cases)

    def texts(t, row):
        return [t["names"][v] if i in (1, 5, 7) else v for i, v in enumerate(row)]

    bad = []
    for i, (a, b) in enumerate(zip(got["rows"], golden["rows"])):
        a, b = texts(got, a), texts(golden, b)
        if a != b:
            bad.append(i)
            if len(bad) <= 20:
                print(f"descriptor {i}: {DC.show(cases[i])}\n   recorded [variant rc, name, tiles, workspace, wgrad rc, name, rc, name] {b}\n   library  {a}")
    assert not bad, f"{len(bad)} of {len(cases)} descriptors answer differently than in the build of {golden['built_from']} (first: {bad[:20]})"
