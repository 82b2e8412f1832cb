"""teHmmEval -- the reference's bin/teHmmEval.py: decode a data set with a trained model, print its score and
optionally write the per-row files.  A MultitrackCfg model is decoded by CYK on the device (cfgEval: --bed and --bic;
--slice bounds the cubic work; --maxPost, --pd, --ed and --segment are refused before data is loaded).

Same positionals, options, defaults and errors as the reference (teHmmEval.py:25-105).  Tracks are loaded through
TrackData.loadTrackData, the model is read by modelIO, every table of a run is evaluated in one fused launch per ratio
group and the lines of --bed, --pd and --ed are formatted on the device (MultitrackHmm.evalToFiles).  --numThreads and
--proc are accepted and ignored: the GPU is the parallelism.  --chroms (the recipe spells it --chrom, which argparse
takes as a prefix): every line of that file is one job over the regions inside it; the jobs run one after the other in
this process and every output file is the concatenation of the jobs' files in job order, as parallelDispatch leaves
them (teHmmEval.py:312-383)."""
import argparse
import copy
import logging
import math
import os
import shutil
import sys
import tempfile

from .common import logger
from .output import getPosteriorsMask, writeBic

MAXINT = sys.maxsize


def parseArgs(argv):
    parser = argparse.ArgumentParser(
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
        description="Evaluate a given data set with a trained HMM. Display the log probability of the input data given "
        "the model, and optionally output the most likely sequence of hidden states.")
    parser.add_argument("tracksInfo", help="Path of Tracks Info file containing paths to genome annotation tracks")
    parser.add_argument("inputModel", help="Path of hmm created with teHmmTrain.py")
    parser.add_argument("bedRegions", help="Intervals to process")
    parser.add_argument("--bed", help="path of file to write viterbi output to (most likely sequence of hidden states)",
                        default=None)
    parser.add_argument("--numThreads", help="Accepted for compatibility: the tables of a run share one launch",
                        type=int, default=1)
    parser.add_argument("--slice", help="Make sure that regions are sliced to a maximum length of the given value. "
                        "When 0, no slicing is done", type=int, default=0)
    parser.add_argument("--segment", help="Use the intervals in bedRegions as segments which each count as a single "
                        "column for evaluattion.  Note the model should have been trained with the --segment option "
                        "pointing to this same bed file.", action="store_true", default=False)
    parser.add_argument("--segLen", help="Effective segment length used for normalizing input segments (specifying 0 "
                        "means no normalization applied)", type=int, default=0)
    parser.add_argument("--maxPost", help="Use maximum posterior decoding instead of Viterbi for evaluation",
                        action="store_true", default=False)
    parser.add_argument("--pd", help="Output BED file for posterior distribution. Must be used in conjunction with "
                        "--pdStates (View on the browser via bedGraphToBigWig)", default=None)
    parser.add_argument("--pdStates", help="comma-separated list of state names to use for computing posterior "
                        "distribution.  For example:  --pdStates inside,LTR_left,LTR_right will compute the "
                        "probability, for each observation, that the hidden state is inside OR LTR_left OR LTR_right.  "
                        "Must be used with --pd to specify output file.", default=None)
    parser.add_argument("--bic", help="save Bayesian Information Criterion (BIC) score in given file", default=None)
    parser.add_argument("--ed", help="Output BED file for emission distribution. Must be used in conjunction with "
                        "--edStates (View on the browser via bedGraphToBigWig)", default=None)
    parser.add_argument("--edStates", help="comma-separated list of state names to use for computing emission "
                        "distribution.  If more than one state is selected, this is not a distribution, but a sum of "
                        "distributions (and values can exceed 1).  Mostly for debugging purposes. Note output in LOG",
                        default=None)
    parser.add_argument("--chroms", help="list of chromosomes, or regions, to run one after the other (in BED format). "
                        "input regions will be intersected with each line in this file, and the result will "
                        "correspsond to an individual job", default=None)
    parser.add_argument("--proc", help="Accepted for compatibility (use in conjunction with --chroms): the jobs run one "
                        "after the other on the one GPU", type=int, default=1)
    parser.add_argument("--logLevel", help="Logging level of the package's logger", default=None)
    args = parser.parse_args(argv)
    checkArgs(args)
    return args


def checkArgs(args):
    """The conflicts teHmmEval.py:94-105 raises on."""
    if args.slice <= 0:
        args.slice = MAXINT
    elif args.segment is True:
        raise RuntimeError("--slice and --segment options are not compatible at this time")
    if (args.pd is not None) ^ (args.pdStates is not None):
        raise RuntimeError("--pd requires --pdStates and vice versa")
    if (args.ed is not None) ^ (args.edStates is not None):
        raise RuntimeError("--ed requires --edStates and vice versa")
    if args.bed is None and (args.pd is not None or args.ed is not None):
        raise RuntimeError("Both --ed and --pd only usable in conjunction with --bed")


def slicedIntervals(bedIntervals, chunkSize):
    """teHmmEval.py:277-292, its quirk included: the slices of an interval start at sliceNo * chunkSize, not at the
    interval's start plus that; the last slice keeps the interval's end."""
    for interval in bedIntervals:
        iLen = interval[2] - interval[1]
        if iLen <= chunkSize:
            yield interval
        else:
            nCuts = int(math.ceil(float(iLen) / float(chunkSize)))
            for sliceNo in range(nCuts):
                sInt = list(copy.deepcopy(interval))
                sInt[1] = sliceNo * chunkSize
                if sliceNo < nCuts - 1:
                    sInt[2] = sInt[1] + chunkSize
                assert sInt[2] > sInt[1]
                yield tuple(sInt)


def chromJobs(regions, chromIntervals, intersect=None):
    """The jobs of --chroms (teHmmEval.py:323-341): per line of the chroms file (sorted by chrom and start) the records
    of the region file inside it -- intersectBed -a regions -b line | sortBed, all columns kept -- or nothing for a
    line no region touches.  [(line, records)] in job order."""
    from . import masking
    if intersect is None:
        intersect = masking.intersectIntervals
    jobs = []
    for line in sorted(chromIntervals, key=lambda r: (r[0], int(r[1]))):
        line = (line[0], int(line[1]), int(line[2]))
        records = masking.sortIntervals(intersect(regions, [line]))
        if len(records) > 0:
            jobs.append((line, records))
    return jobs


def runEval(args, out=None):
    """One run of the tool on args.bedRegions (teHmmEval.py:113-236)."""
    from . import modelIO, trackIO
    from .cfg import MultitrackCfg
    from .track import TrackData
    out = sys.stdout if out is None else out
    logger.info("loading model %s" % args.inputModel)
    model = modelIO.loadModel(args.inputModel)
    isCfg = isinstance(model, MultitrackCfg)
    if isCfg:
        # teHmmEval.py:117-119; the grammar model has no posterior or emission column either
        if args.maxPost is True:
            raise RuntimeError("--maxPost not supported on CFG models")
        if args.pd is not None or args.ed is not None:
            raise RuntimeError("--pd and --ed not supported on CFG models")
        if args.segment is True:
            raise RuntimeError("--segment not supported on CFG models")

    if args.segLen > 0:
        assert args.segment is True
        model.getEmissionModel().effectiveSegmentLength = args.segLen

    logger.info("loading target intervals from %s" % args.bedRegions)
    mergedIntervals = trackIO.getMergedBedIntervals(args.bedRegions, ncol=3)
    if mergedIntervals is None or len(mergedIntervals) < 1:
        raise RuntimeError("Could not read any intervals from %s" % args.bedRegions)
    choppedIntervals = [x for x in slicedIntervals(mergedIntervals, args.slice)]

    segIntervals = None
    if args.segment is True:
        logger.info("loading segment intervals from %s" % args.bedRegions)
        segIntervals = trackIO.readBedColumns(args.bedRegions, sort=True)

    logger.info("loading tracks %s" % args.tracksInfo)
    trackData = TrackData()
    trackData.loadTrackData(args.tracksInfo, choppedIntervals, model.getTrackList(), segmentIntervals=segIntervals,
                            allowAlignment=isCfg)
    if isCfg:
        return cfgEval(args, model, trackData, out)

    logger.info("running %s algorithm" % ("posterior decoding" if args.maxPost is True else "viterbi"))
    pdMask = edMask = None
    if args.pd is not None:
        pdMask = getPosteriorsMask(args.pdStates, model)
        assert model.getEmissionModel().getNumStates() == len(pdMask)
    if args.ed is not None:
        edMask = getPosteriorsMask(args.edStates, model)
        assert model.getEmissionModel().getNumStates() == len(edMask)
    scores, _ = model.evalToFiles(trackData, bedPath=args.bed, pdPath=args.pd, pdMask=pdMask, edPath=args.ed,
                                  edMask=edMask, maxPost=args.maxPost)
    totalScore = 0
    totalDatapoints = 0
    for table, score in zip(trackData.getTrackTableList(), scores):
        totalScore += score
        if args.bed is not None or args.pd is not None:
            totalDatapoints += len(table) * table.getNumTracks()

    out.write("Viterbi (log) score: %f\n" % totalScore)
    if getattr(model, "current_iteration", None) is not None:
        out.write("Number of EM iterations: %d\n" % model.current_iteration)
    if args.bic is not None:
        writeBic(args.bic, model, totalScore, totalDatapoints)
    return 0


def cfgEval(args, model, trackData, out):
    """The CFG branch of teHmmEval.py:158-236: CYK over all tables in one device call, the --bed file through the
    writers of the HMM branch with the trace as the state rows.  The work grows with the cube of an interval's
    length: --slice bounds it."""
    from .output import statesToBed
    logger.info("running CYK algorithm")
    if args.bed is not None:
        open(args.bed, "w").close()
    totalScore = 0
    totalDatapoints = 0
    names = None
    if model.getStateNameMap() is not None:
        names = [model.getStateNameMap().getMapBack(i) for i in range(model.getEmissionModel().getNumStates())]
    for table, (score, states) in zip(trackData.getTrackTableList(), model.viterbi(trackData)):
        totalScore += score
        if args.bed is not None:
            with open(args.bed, "a") as f:
                f.write("#Viterbi Score: %f\n" % score)
            if names is not None:
                states = [model.getStateNameMap().getMap(s) for s in states]
            statesToBed(table, [int(s) for s in states], args.bed, stateNames=names)
            totalDatapoints += len(table) * table.getNumTracks()
    out.write("Viterbi (log) score: %f\n" % totalScore)
    if args.bic is not None:
        writeBic(args.bic, model, totalScore, totalDatapoints)
    return 0


def _append_file(src, dst, first):
    with open(src, "rb") as f, open(dst, "wb" if first else "ab") as g:
        shutil.copyfileobj(f, g)


def parallelDispatch(args, out=None):
    """--chroms: one run per job of chromJobs, each on a region file of its own; the jobs' output files are joined in
    job order."""
    from . import masking, trackIO
    jobs = chromJobs(masking.readBed(args.bedRegions), trackIO.readBedIntervals(args.chroms, sort=True))
    tmp = tempfile.mkdtemp(prefix="tehmm_eval_")
    try:
        for n, (_, records) in enumerate(jobs):
            job = copy.copy(args)
            job.chroms = None
            job.bedRegions = os.path.join(tmp, "regions_%d.bed" % n)
            masking.writeBed(records, job.bedRegions)
            for opt in ("bed", "pd", "ed", "bic"):
                if getattr(args, opt) is not None:
                    setattr(job, opt, os.path.join(tmp, "%s_%d" % (opt, n)))
            runEval(job, out)
            for opt in ("bed", "pd", "ed", "bic"):
                if getattr(args, opt) is not None:
                    _append_file(getattr(job, opt), getattr(args, opt), n == 0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


def main(argv=None, out=None):
    """The command line of bin/teHmmEval.py: tracksInfo inputModel bedRegions [options]."""
    args = parseArgs(sys.argv[1:] if argv is None else argv)
    if args.logLevel is not None:
        logger.setLevel(getattr(logging, args.logLevel.upper()))
    if args.chroms is not None:
        return parallelDispatch(args, out)
    return runEval(args, out)


if __name__ == "__main__":
    sys.exit(main())
