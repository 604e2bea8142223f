"""svim-asm-small, --left_align and svim-asm-small-compare held to the contigs they must rebuild, on the device: the checks of
tests/test_small_rebuild_host.py (see there for what is asserted) with the real kernels — svx_cigar_mismatch over the
readers' CIGAR pool in HBM (BAM input) and over the host's words (SAM input), svx_cigar_extract on both of its paths,
svx_indel_shift under every hand-over, svx_cover_single, the BGZF encoder, svx_cover_query and svx_variant_replay — on the
cases of tests/rebuild_cases.py, judged by tests/rebuild_judge.py."""
import os

import pytest

from svim_asm_amd import _lib, small_cli
from tests import rebuild_cases as RC, tabix_reader as TR, test_small_rebuild_host as R
from tests.test_small_rebuild_host import rebuild_dir  # noqa: F401  (the session's directory of inputs and runs)

pytestmark = pytest.mark.gpu

SMALL_BATCH_DEFAULT = 1 << 23
HAND_OVERS = {"wave-form": 0, "lane-form": _lib.SHIFT_LANES_ONLY}
SHIFTED = RC.LEFTMOST + ("random-1",)


def _alternate(name):
    return R.KINDS[RC.NAMES.index(name) % 2]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("left_align", R.MODES, ids=("asis", "left"))
@pytest.mark.parametrize("name", RC.NAMES)
def test_rebuild_on_the_device(name, left_align, kind, rebuild_dir, svx_ctx):  # noqa: F811
    out, vcf, _ = R.plain_run(rebuild_dir, "device", name, left_align, kind)
    records, summary = R.check_run(name, left_align, out)
    R.check_named_expectations(name, left_align, records)
    if left_align:
        assert [l.split("\t")[:5] for l in R.snv_lines(vcf)] == [l.split("\t")[:5] for l in R.snv_lines(R.plain_run(rebuild_dir, "device", name, False, kind)[1])]
    if kind == "bam":
        assert R.plain_run(rebuild_dir, "device", name, left_align, "sam")[1:] == R.plain_run(rebuild_dir, "device", name, left_align, "bam")[1:]


@pytest.mark.parametrize("hand_over", sorted(HAND_OVERS))
@pytest.mark.parametrize("name", SHIFTED)
def test_left_align_under_every_hand_over(name, hand_over, rebuild_dir, svx_ctx, tmp_path):  # noqa: F811
    kind = _alternate(name)
    _, vcf, summary = R.plain_run(rebuild_dir, "device", name, True, kind)   # (the default hand-over, judged above)
    ctx = _lib.default_context(0)
    ctx.set_shift_lane_steps(HAND_OVERS[hand_over])
    try:
        out = str(tmp_path / "out")
        assert small_cli.main(R.argv_of(rebuild_dir, name, kind, True, out)) == 0
    finally:
        ctx.set_shift_lane_steps(-1)
    records, _ = R.check_run(name, True, out)
    R.check_named_expectations(name, True, records)
    assert R.read_outputs(out) == (vcf, summary)


@pytest.mark.parametrize("name", RC.NAMES)
def test_several_batches_give_the_same_bytes_on_the_device(name, rebuild_dir, svx_ctx, tmp_path, monkeypatch):  # noqa: F811
    kind = _alternate(name)
    _, vcf, summary = R.plain_run(rebuild_dir, "device", name, True, kind)
    calls, entry = [], _lib.Context.cigar_mismatch

    def counted(self, *args, **kw):
        calls.append(1)
        return entry(self, *args, **kw)
    monkeypatch.setattr(_lib.Context, "cigar_mismatch", counted)
    out = str(tmp_path / "batches")
    assert small_cli.main(R.argv_of(rebuild_dir, name, kind, True, out, ["--batch_bases", str(R.batch_limit(name))])) == 0
    assert R.read_outputs(out) == (vcf, summary) and len(calls) >= 3


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_streaming_cigar_path_gives_the_same_bytes(name, rebuild_dir, svx_ctx, tmp_path):  # noqa: F811
    kind = _alternate(name)
    _, vcf, summary = R.plain_run(rebuild_dir, "device", name, True, kind)
    ctx = _lib.default_context(0)
    ctx.set_small_batch_ops(0)
    try:
        out = str(tmp_path / "streaming")
        assert small_cli.main(R.argv_of(rebuild_dir, name, kind, True, out)) == 0
    finally:
        ctx.set_small_batch_ops(SMALL_BATCH_DEFAULT)
    assert R.read_outputs(out) == (vcf, summary)


@pytest.mark.parametrize("name", RC.NAMES)
def test_bgzip_output_reads_back(name, rebuild_dir, svx_ctx, tmp_path, monkeypatch):  # noqa: F811
    kind = _alternate(name)
    _, vcf, summary = R.plain_run(rebuild_dir, "device", name, False, kind)
    monkeypatch.setenv("SVX_VCF_BGZF_DEVICE", "1")
    out = str(tmp_path / "z")
    assert small_cli.main(R.argv_of(rebuild_dir, name, kind, False, out, ["--bgzip_output"])) == 0
    assert sorted(os.listdir(out)) == ["small.vcf.gz", "small.vcf.gz.tbi", "summary.json"]
    assert open(os.path.join(out, "summary.json")).read() == summary
    blob, text = open(os.path.join(out, "small.vcf.gz"), "rb").read(), vcf.encode()
    TR.check_bgzf(blob, text)
    reader = TR.Reader(blob, open(os.path.join(out, "small.vcf.gz.tbi"), "rb").read())
    for contig in RC.ORDER:
        for beg, end in ((0, 1 << 29), (1000, 1000 + RC.T), (20000, 20001)):
            assert reader.query(contig, beg, end) == TR.brute(text, contig, beg, end)


@pytest.mark.parametrize("left_align", R.MODES, ids=("asis", "left"))
@pytest.mark.parametrize("name", RC.COMPARED)
def test_compare_closes_the_loop_on_the_device(name, left_align, rebuild_dir, svx_ctx, monkeypatch):  # noqa: F811
    calls, entry = [], _lib.Context.variant_replay

    def counted(self, *args, **kw):
        calls.append(1)
        return entry(self, *args, **kw)
    monkeypatch.setattr(_lib.Context, "variant_replay", counted)
    summary = R.check_compare(rebuild_dir, "device", name, left_align)
    assert len(calls) >= min(2, summary["clusters"]["replayed"])
