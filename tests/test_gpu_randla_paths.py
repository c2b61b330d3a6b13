"""GPU: every attention kernel and per-point Linear path of csrc/randla.hip ONE AT A TIME on the MI355X, through
``ops.randla_forward`` with precomputed index tables -- the bodies and the case table of tests/randla_cases.py (shared with
tests/test_emulated_randla_paths.py, which runs the rows of at most about 2 000 rows per level on the host emulator, and with
tests/test_randla_cases_can_fail.py, which shows that each row's bound rejects a faulty layer).  A test is one class in one
situation: the width under test is the LAST encoder layer of a one- or two-layer net; tiny (one cloud of 16 points, and three
clouds below 64 tiles: no XCD remap), ragged (three odd clouds: tiles straddle clouds, partial last tile, remap with a
remainder), remap with one cloud (32 chunks), loop (a row count just above the class's grid cap at THIS device's CU count: some
worker takes a second tile), and in every row the same forward with a reversed and a random ``tile_order``, bit for bit, in a
workspace of NaN bytes and into an output of NaN.  Logits
against ``oracle.randlanet_ref.forward`` in FLOAT64 within max(1e-5, 4 e32) <= 1e-4 (pt_cases.judge); two runs, a workspace of NaN
bytes, other clouds beside a cloud and the refusals for equality.  The measured figures of every comparison are appended to the
per-YAML parity record of tests/test_gpu_configs.py (family ``randla_paths``); the table is profiles/randla_gpu_tests.md.

Measured on an MI355X (256 CUs): all 46 comparisons inside max(1e-5, 4 e32), the closest (stage512-tiny2) at 0.48 of it with
max |delta| 1.28e-5 = 1.92 e32; every exact check bit for bit; a kernel trace of this file matched the launches that
randla_cases.plan derives for every test, launch for launch (profiles/randla_gpu_tests.md).  The 59 tests take 16.8 s together, the slowest (stage512-loop,
8199 one-point tiles: mostly its float64 reference) 4.0 s."""
import pytest

import randla_cases as G
from test_gpu_configs import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def report(**kv):
    print(" ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items()), flush=True)
    record(kv.pop("name"), family="randla_paths", **kv)


@pytest.mark.parametrize("index", range(len(G.CASES)), ids=G.CASE_IDS)
def test_one_class_in_one_situation_against_float64_and_under_a_tile_order(index):
    G.check_case(DEV, index, report)


@pytest.mark.parametrize("index", G.EXACT, ids=[G.CASE_IDS[i] for i in G.EXACT])
def test_two_runs_nan_workspace_and_other_clouds_bit_for_bit(index):
    G.check_exact(DEV, index)


def test_refused_configurations_shapes_and_dtypes():
    G.check_refusals(DEV)
