"""Random walks over the whole stream API -- the four batch entry points with random bindings (consensus codes, change list, species
call, the call's change list), refused batches, table / rank / reads, the breadth and depth queries with export and import, table_add,
reset, the packed toggle, flush / sync / wait / drain -- on one stream per walk, against the CPU model of tests/stream_model.py, which
is the oracle chained batch by batch plus the restatements of the single-feature tests.  tests/test_gpu_fuzz.py walks the rows and
the table of a single-species stream; these walk what the stream has gained since, in three worlds: a reference with every storage
class (`classes`), three species (`species`) and a clone tree whose batches rank on their candidates (`tree`).

Four walks per world, at most 40 ops and 1 500 reads each; tests/test_stream_model_cpu.py pins what the committed walks contain.
SKX_TEST_SEED selects another set of walks.  A failing walk prints itself as `replay(world, ops)`: paste it here as a fixed test."""
import os

import pytest

import stream_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _references(gpu):
    yield
    sm.close_references()


def _walks(world):
    base = int(os.environ.get("SKX_TEST_SEED", str(sm.SEED_BASE)))
    infos = []
    for seed in sm.seeds(world, base):
        ops = sm.plan(world, seed)
        info = sm.run(world, ops, seed=seed)
        st = info["stats"]
        print(f"walk {world} seed {seed}: {info['executed']} ops, {info['total']} reads, {info['seconds']:.2f} s, create {ops[0]}, passes",
              st["passes"], "shared", st["passes_shared"], "unshared", st["groups_unshared"], "compact", st["batches_compact"], "full",
              st["batches_full"], "bound", info["bound"], "passes of a bound batch", info["bound_passes"])
        assert info["executed"] == len(ops) and info["reads"] == info["stats_reads"]
        infos.append(info)
    assert sum(i["total"] for i in infos) > 2000  # (the walks really pushed reads through)
    assert any(i["bound"] and i["stats"]["passes_shared"] > 0 for i in infos), "no walk with bindings had batches that shared a pass"
    return infos


def test_walks_on_a_reference_of_every_storage_class(gpu):
    _walks("classes")


def test_walks_on_three_species(gpu):
    infos = _walks("species")
    assert max(i["bound_passes"] for i in infos) > 1, "no bound batch was cut into several passes"


def test_walks_on_a_clone_tree(gpu):
    infos = _walks("tree")
    assert sum(i["stats"]["batches_compact"] for i in infos) > 0, "no batch ranked on its candidates"
    assert sum(i["stats"]["batches_full"] for i in infos) > 0, "no batch ranked on every genome"
