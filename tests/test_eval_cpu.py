"""teHmmEval's helpers without a GPU: slicedIntervals and getPosteriorsMask against what the reference's own functions
returned (tests/golden/eval.json, made by make_golden_eval.py), the argument checks, and the job split of --chroms."""
import json
import os

import numpy as np
import pytest

import masking_ref as mr
from conftest import GOLDEN
from tehmm_amd import eval as te
from tehmm_amd.output import getPosteriorsMask
from tehmm_amd.track import CategoryMap


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "eval.json")) as f:
        return json.load(f)


def test_sliced_intervals_match_the_reference(golden):
    assert len(golden["sliced"]) >= 20
    for case in golden["sliced"]:
        intervals = [tuple(iv) for iv in case["intervals"]]
        if case["out"] == "AssertionError":
            with pytest.raises(AssertionError):
                list(te.slicedIntervals(intervals, case["chunk"]))
            continue
        got = [list(x) for x in te.slicedIntervals(intervals, case["chunk"])]
        assert got == case["out"], (case["intervals"], case["chunk"])


def test_sliced_intervals_keep_the_quirk():
    # a slice starts at sliceNo * chunkSize, not at the interval's start plus that
    assert list(te.slicedIntervals([("chr1", 500, 2700)], 1000)) == [
        ("chr1", 0, 1000), ("chr1", 1000, 2000), ("chr1", 2000, 2700)]


class _Em(object):
    def __init__(self, n):
        self.n = n

    def getNumStates(self):
        return self.n


class _Hmm(object):
    def __init__(self, n, names):
        self.em, self.map = _Em(n), None
        if names is not None:
            self.map = CategoryMap(reserved=0)
            for name in names:
                self.map.update(name)

    def getStateNameMap(self):
        return self.map

    def getEmissionModel(self):
        return self.em


def test_posteriors_mask_matches_the_reference(golden):
    assert len(golden["mask"]) >= 8
    for case in golden["mask"]:
        mask = getPosteriorsMask(case["pdStates"], _Hmm(case["n"], case["names"]))
        assert str(mask.dtype) == case["dtype"]
        assert mask.tolist() == case["mask"], case


def _parse(*opts):
    return te.parseArgs(["tracks.xml", "model.mod", "regions.bed"] + list(opts))


def test_argument_checks_raise_the_references_errors():
    with pytest.raises(RuntimeError, match="--slice and --segment options are not compatible at this time"):
        _parse("--slice", "100", "--segment")
    for opts in (("--pd", "x.bed", "--bed", "b.bed"), ("--pdStates", "0", "--bed", "b.bed")):
        with pytest.raises(RuntimeError, match="--pd requires --pdStates and vice versa"):
            _parse(*opts)
    for opts in (("--ed", "x.bed", "--bed", "b.bed"), ("--edStates", "0", "--bed", "b.bed")):
        with pytest.raises(RuntimeError, match="--ed requires --edStates and vice versa"):
            _parse(*opts)
    for opts in (("--pd", "x.bed", "--pdStates", "0"), ("--ed", "x.bed", "--edStates", "0")):
        with pytest.raises(RuntimeError, match="Both --ed and --pd only usable in conjunction with --bed"):
            _parse(*opts)


def test_defaults_and_accepted_options():
    a = _parse()
    assert (a.bed, a.pd, a.pdStates, a.ed, a.edStates, a.bic, a.chroms) == (None,) * 7
    assert a.slice == te.MAXINT and a.segment is False and a.segLen == 0 and a.maxPost is False
    assert a.numThreads == 1 and a.proc == 1
    a = _parse("--numThreads", "8", "--proc", "4", "--chrom", "c.bed", "--slice", "1000", "--bic", "x.bic")
    assert (a.numThreads, a.proc, a.chroms, a.slice, a.bic) == (8, 4, "c.bed", 1000, "x.bic")
    a = _parse("--segment", "--segLen", "100", "--maxPost", "--bed", "b.bed", "--pd", "p", "--pdStates", "1,2")
    assert a.segment is True and a.segLen == 100 and a.maxPost is True and a.pdStates == "1,2"


def _intersect(a, b):
    return mr.carry(a, mr.intersect(a, mr.sort_intervals(b)))


def test_chroms_job_split():
    regions = [("chr2", 100, 900, "r0"), ("chr1", 0, 1000, "r1"), ("chr1", 1500, 3000, "r2"), ("chr10", 5, 50, "r3")]
    chroms = [("chr2", 0, 500), ("chr1", 800, 2000), ("chr3", 0, 100), ("chr1", 0, 100), ("chr1", 2500, 9000)]
    jobs = te.chromJobs(regions, chroms, intersect=_intersect)
    # lines in (chrom, start) order, the line no region touches dropped, records sorted with their other columns
    assert [j[0] for j in jobs] == [("chr1", 0, 100), ("chr1", 800, 2000), ("chr1", 2500, 9000), ("chr2", 0, 500)]
    assert jobs[0][1] == [("chr1", 0, 100, "r1")]
    assert jobs[1][1] == [("chr1", 800, 1000, "r1"), ("chr1", 1500, 2000, "r2")]
    assert jobs[2][1] == [("chr1", 2500, 3000, "r2")]
    assert jobs[3][1] == [("chr2", 100, 500, "r0")]
    assert te.chromJobs(regions, [("chr9", 0, 10)], intersect=_intersect) == []
