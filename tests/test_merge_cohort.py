"""`svim-asm-cohort --gpus N --merge DIR` without a GPU: stubs in the place of the children (cohort._child_command) and of
the merge child (cohort._merge_command), so nothing here loads the library or needs a device."""
import json
import os
import sys

import pytest

from svim_asm_amd import cohort

STUB = r"""
import json, os, sys
plan = json.load(open(os.environ["STUB_PLAN"]))
out = plan["out"]
role = "merge" if sys.argv[1] == "MERGE" else "child"
device = int(sys.argv[sys.argv.index("--device") + 1])
done = sorted(n for n in os.listdir(out) if n.startswith("done_"))
with open(os.path.join(out, "%s_%d_%d.json" % (role, device, os.getpid())), "w") as f:
    json.dump({"argv": sys.argv[1:], "done_before": done, "siblings": os.environ.get("SVX_NODE_PROCESSES")}, f)
with open(os.path.join(out, "done_%s_%d_%d" % (role, device, os.getpid())), "w") as f:
    f.write("done")
sys.exit(plan.get("status", {}).get("merge" if role == "merge" else str(device), 0))
"""


@pytest.fixture
def stub(tmp_path, monkeypatch):
    out = tmp_path / "stub_out"
    out.mkdir()
    plan_path = tmp_path / "stub_plan.json"

    def set_plan(**plan):
        plan_path.write_text(json.dumps(dict(plan, out=str(out))))
    set_plan()
    monkeypatch.setenv("STUB_PLAN", str(plan_path))
    real_merge_command = cohort._merge_command
    monkeypatch.setattr(cohort, "_child_command", lambda mode, share, genome, device, rest:
                        [sys.executable, "-c", STUB, mode, share, genome, "--device", str(device)] + list(rest))
    # the merge child: the stub, behind it the arguments the real command would get
    monkeypatch.setattr(cohort, "_merge_command", lambda *a: [sys.executable, "-c", STUB, "MERGE"] + real_merge_command(*a)[2:])

    def records(role):
        return [json.load(open(out / n)) for n in sorted(os.listdir(out)) if n.startswith(role + "_")]
    return set_plan, records


def _manifest(tmp_path, n):
    path = tmp_path / "cohort.tsv"
    path.write_text("".join("%s s%d_h0.bam s%d_h1.bam\n" % (tmp_path / ("wd%d" % k), k, k) for k in range(n)))
    return str(path)


def test_children_keep_their_tables_and_one_merge_child_follows(tmp_path, stub):
    set_plan, records = stub
    out_dir = str(tmp_path / "merged")
    assert cohort.main(["diploid", _manifest(tmp_path, 5), "ref.fa", "--gpus", "2", "--devices", "3,1", "--merge", out_dir,
                        "--max_edit_distance", "77", "--symbolic_alleles", "--min_sv_size", "50", "--cohort_workers", "2"]) == 0
    children, merges = records("child"), records("merge")
    assert len(children) == 2 and len(merges) == 1
    for rec in children:
        assert rec["argv"].count("--keep_candidates") == 1
        assert "--merge" not in rec["argv"] and out_dir not in rec["argv"]
        assert not any(n.startswith("done_merge") for n in rec["done_before"])
    m = merges[0]
    # started when both children were gone, alone, on the first listed device
    assert len([n for n in m["done_before"] if n.startswith("done_child")]) == 2
    assert m["siblings"] == "1"
    a = m["argv"][1:]
    assert a[:2] == [out_dir, "ref.fa"] and a[2:7] == [str(tmp_path / ("wd%d" % k)) for k in range(5)]  # manifest order
    assert a[a.index("--device") + 1] == "3"
    assert a[a.index("--max_edit_distance") + 1] == "77" and a[a.index("--partition_max_distance") + 1] == "1000"
    assert "--symbolic_alleles" in a and "--min_sv_size" not in a and "--bgzip_output" not in a and "--cohort_workers" not in a


def test_keep_candidates_given_by_hand_is_not_doubled(tmp_path, stub):
    set_plan, records = stub
    assert cohort.main(["haploid", str(_haploid_manifest(tmp_path)), "ref.fa", "--gpus", "1", "--keep_candidates", "--merge",
                        str(tmp_path / "m")]) == 0
    assert records("child")[0]["argv"].count("--keep_candidates") == 1 and len(records("merge")) == 1


def _haploid_manifest(tmp_path):
    path = tmp_path / "haploid.tsv"
    path.write_text("%s a.bam\n%s b.bam\n" % (tmp_path / "a", tmp_path / "b"))
    return path


def test_no_merge_child_when_a_child_failed(tmp_path, stub, caplog):
    set_plan, records = stub
    set_plan(status={"1": 3})
    import logging
    with caplog.at_level(logging.INFO):
        assert cohort.main(["diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2", "--merge", str(tmp_path / "m")]) == 3
    assert len(records("child")) == 2 and records("merge") == []
    assert any("MERGE: not attempted" in r.getMessage() for r in caplog.records)


def test_the_parents_status_includes_the_merge_childs(tmp_path, stub):
    set_plan, records = stub
    set_plan(status={"merge": 5})
    assert cohort.main(["diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2", "--merge", str(tmp_path / "m")]) == 5
    assert len(records("child")) == 2 and len(records("merge")) == 1


def test_without_merge_nothing_changes(tmp_path, stub):
    set_plan, records = stub
    assert cohort.main(["diploid", _manifest(tmp_path, 4), "ref.fa", "--gpus", "2"]) == 0
    assert all("--keep_candidates" not in r["argv"] for r in records("child")) and records("merge") == []
