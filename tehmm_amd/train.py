"""teHmmTrain -- the reference's bin/teHmmTrain.py: build a MultitrackHmm from track files and train it supervised
(state names of the training BED), by Baum-Welch, or semi-supervised -- Baum-Welch from user start / transition /
emission files (--init*Probs), with entries pinned through every iteration (--force*Probs); or, with --cfg
--supervised, a MultitrackCfg whose --pairStates emit pairs of columns under the --saPrior confidence in the track
list's alignment track.

Same options, the same conflicts between them and the same default for transMatEpsilons as the reference
(teHmmTrain.py:188-225).  Tracks are loaded through TrackData.loadTrackData, the model is written by modelIO.  Where
no random draw is involved (--flatEm, --supervised, init / force files) the model is the reference's; replicates
(--reps) run one after the other on the one GPU and the best is the one with the highest last forward
log-probability (teHmmTrain.py:294-306)."""
import argparse
import logging
import random
import sys

import numpy as np

from .common import LOGZERO, logger
from .hmm import _py2_gt, _user_lines


def parseArgs(argv):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                     description="Create a teHMM")
    parser.add_argument("tracksInfo", help="Path of Tracks Info file containing paths to genome annotation tracks")
    parser.add_argument("trainingBed", help="Path of BED file containing genome regions to train model on.  If "
                        "--supervised is used, the names in this bed file will be treated as the true annotation "
                        "(otherwise it is only used for interval coordinates)")
    parser.add_argument("outputModel", help="Path of output hmm")
    parser.add_argument("--numStates", help="Number of states in model", type=int, default=2)
    parser.add_argument("--iter", help="Number of EM iterations", type=int, default=100)
    parser.add_argument("--supervised", help="Use name (4th) column of <traingingBed> for the true hidden states of "
                        "the model.  Transition parameters will be estimated directly from this information rather "
                        "than EM.  NOTE: The number of states will be determined from the bed.",
                        action="store_true", default=False)
    parser.add_argument("--cfg", help="Use Context Free Grammar instead of HMM.  Only works with --supervised",
                        action="store_true", default=False)
    parser.add_argument("--saPrior", help="Confidence in self alignment track for CFG.  Probability of pair emission "
                        "is multiplied by this number if the bases are aligned and its complement if bases are not "
                        "aligned. Must be between [0,1].", default=0.95, type=float)
    parser.add_argument("--pairStates", help="Comma-separated list of states (from trainingBed) that are treated as "
                        "pair-emitors for the CFG", default=None)
    parser.add_argument("--emFac", help="Normalization factor for weighting emission probabilities because when "
                        "there are many tracks, the transition probabilities can get totally lost. 0 = no "
                        "normalization. 1 = divide by number of tracks.  k = divide by number of tracks / k",
                        type=int, default=0)
    parser.add_argument("--initTransProbs", help="Path of text file where each line has three entries: FromState "
                        "ToState Probability.  This file (all other transitions get probability 0) is used to "
                        "specifiy the initial transition model.  The names and number of states will be initialized "
                        "according to this file (overriding --numStates)", default=None)
    parser.add_argument("--fixTrans", help="Do not learn transition parameters (best used with --initTransProbs)",
                        action="store_true", default=False)
    parser.add_argument("--initEmProbs", help="Path of text file where each line has four entries: State Track "
                        "Symbol Probability.  This file (all other emissions get probability 0) is used to specifiy "
                        "the initial emission model. All states specified in this file must appear in the file "
                        "specified with --initTransProbs (but not vice versa).", default=None)
    parser.add_argument("--fixEm", help="Do not learn emission parameters (best used with --initEmProbs)",
                        action="store_true", default=False)
    parser.add_argument("--initStartProbs", help="Path of text file where each line has two entries: State "
                        "Probability.  This file (all other start probs get probability 0) is used to specifiy the "
                        "initial start dist. All states specified in this file must appear in the file specified "
                        "with --initTransProbs (but not vice versa).", default=None)
    parser.add_argument("--fixStart", help="Do not learn start parameters (best used with --initStartProbs)",
                        action="store_true", default=False)
    parser.add_argument("--forceTransProbs", help="Path of text file where each line has three entries: FromState "
                        "ToState Probability. These transition probabilities will override any learned probabilities "
                        "after each training iteration (unspecified will not be set to 0 in this case. the learned "
                        "values will be kept, but normalized as needed)", default=None)
    parser.add_argument("--forceEmProbs", help="Path of text file where each line has four entries: State Track "
                        "Symbol Probability. These emission probabilities will override any learned probabilities "
                        "after each training iteration (unspecified will not be set to 0 in this case. the learned "
                        "values will be kept, but normalized as needed.)", default=None)
    parser.add_argument("--flatEm", help="Use a flat emission distribution as a baseline.  If not specified, the "
                        "initial emission distribution will be randomized by default.  Emission probabilities "
                        "specified with --initEmpProbs or --forceEmProbs will never be affected by randomizaiton.",
                        action="store_true", default=False)
    parser.add_argument("--emRandRange", help="When randomly initialzing an emission distribution, constrain the "
                        "values to the given range (pair of comma-separated numbers).  Overridden by --initEmProbs "
                        "and --forceEmProbs when applicable. Completely overridden by --flatEm (which is equivalent "
                        "to --emRandRange .5,.5.). Actual values used will always be normalized.", default="0.2,0.8")
    parser.add_argument("--segment", help="Bed file of segments to treat as single columns for HMM (ie as created "
                        "with the segmenter).  IMPORTANT: this file must cover the same regions as the traininBed "
                        "file.", default=None)
    parser.add_argument("--segLen", help="Effective segment length used for normalizing input segments (specifying 0 "
                        "means no normalization applied)", type=int, default=0)
    parser.add_argument("--seed", help="Seed for random number generator which will be used to initialize emissions "
                        "(if --flatEM and --supervised not specified)", default=None, type=int)
    parser.add_argument("--reps", help="Number of replicates (with different random initializations) to run. The "
                        "replicate with the highest likelihood will be chosen for the output", default=1, type=int)
    parser.add_argument("--numThreads", help="Accepted for compatibility: replicates run one after the other on the "
                        "one GPU", type=int, default=1)
    parser.add_argument("--emThresh", help="Threshold used for convergence in baum welch training.  IE delta log "
                        "likelihood must be bigger than this number (which should be positive) for convergence",
                        type=float, default=0.001)
    parser.add_argument("--saveAllReps", help="Save all replicates (--reps) models to disk, instead of just the best "
                        "one. Format is <outputModel>.repN.  There will be --reps -1 such models saved as the best "
                        "output counts as a replicate", action="store_true", default=False)
    parser.add_argument("--maxProb", help="Gaussian distributions and/or segment length corrections can cause "
                        "probability to *decrease* during BW iteration.  Use this option to remember the parameters "
                        "with the highest probability rather than returning the parameters after the final "
                        "iteration.", action="store_true", default=False)
    parser.add_argument("--maxProbCut", help="Use with --maxProb option to stop training if a given number of "
                        "iterations go by without hitting a new maxProb", default=None, type=int)
    parser.add_argument("--transMatEpsilons", help="By default, epsilons are added to all transition probabilities to "
                        "prevent converging on 0 due to rounding error only for fully unsupervised training.  Use "
                        "this option to force this behaviour for supervised and semisupervised modes",
                        action="store_true", default=False)
    parser.add_argument("--logLevel", help="Logging level of the package's logger", default=None)
    args = parser.parse_args(argv)
    checkArgs(args)
    return args


def checkArgs(args):
    """The conflicts teHmmTrain.py:188-225 raises on, and its default for transMatEpsilons."""
    if args.cfg is True:
        if args.supervised is not True:
            raise RuntimeError("--cfg only works with --supervised")
        if not 0. <= args.saPrior <= 1.:
            raise RuntimeError("--saPrior must be between [0,1]")
        if (args.initTransProbs is not None or args.fixTrans is True or args.initEmProbs is not None or
                args.fixEm is True or args.initStartProbs is not None):
            raise RuntimeError("--initTransProbs, --fixTrans, --initEmProbs, --fixEm, --initStartProbs are not "
                               "compatible with --cfg.")
        if args.forceTransProbs is not None or args.forceEmProbs is not None:
            raise RuntimeError("--forceTransProbs and --forceEmProbs are not compatible with --cfg")
    elif args.pairStates is not None:
        raise RuntimeError("--pairStates needs --cfg")
    if args.fixTrans is True and args.supervised is True:
        raise RuntimeError("--fixTrans option not compatible with --supervised")
    if args.fixEm is True and args.supervised is True:
        raise RuntimeError("--fixEm option not compatible with --supervised")
    if args.flatEm is True and args.supervised is False and args.initEmProbs is None and args.initTransProbs is None:
        raise RuntimeError("--flatEm must be used with --initEmProbs and or --initTransProbs")
    if args.initEmProbs is not None and args.initTransProbs is None:
        raise RuntimeError("--initEmProbs can only be used in conjunction with --initTransProbs")
    if args.emRandRange is not None and not isinstance(args.emRandRange, tuple):
        try:
            toks = args.emRandRange.split(",")
            assert len(toks) == 2
            args.emRandRange = (float(toks[0]), float(toks[1]))
        except Exception:
            raise RuntimeError("Invalid --emRandRange specified")
    if args.transMatEpsilons is False:
        # on by default for plain unsupervised training only
        args.transMatEpsilons = (args.supervised is False and args.initTransProbs is None and
                                 args.forceTransProbs is None)
    if args.segment is None and args.segLen > 0:
        raise RuntimeError("--segLen can only be used with --segment")
    if args.segLen <= 0:
        args.segLen = None
    elif args.segLen != 1:
        logger.warning("--segLen should be 0 (no correction) or 1 (base correction).  Values > 1 may cause bias.")


def main(argv=None):
    """The command line of bin/teHmmTrain.py: tracksInfo trainingBed outputModel [options]."""
    from . import compare, modelIO, trackIO
    from .track import TrackData
    args = parseArgs(sys.argv[1:] if argv is None else argv)
    if args.logLevel is not None:
        logger.setLevel(getattr(logging, args.logLevel.upper()))

    logger.info("loading training intervals from %s" % args.trainingBed)
    mergedIntervals = trackIO.getMergedBedIntervals(args.trainingBed, ncol=3)
    if mergedIntervals is None or len(mergedIntervals) < 1:
        raise RuntimeError("Could not read any intervals from %s" % args.trainingBed)

    segIntervals = None
    if args.segment is not None:
        logger.info("loading segment intervals from %s" % args.segment)
        segIntervals = trackIO.readBedColumns(args.segment, sort=True)
        try:
            compare.checkExactOverlap(trackIO.readBedIntervals(args.trainingBed), trackIO.readBedIntervals(args.segment))
        except Exception:
            raise RuntimeError("bed file passed with --segments option must exactly overlap trainingBed")

    logger.info("loading tracks %s" % args.tracksInfo)
    trackData = TrackData()
    trackData.loadTrackData(args.tracksInfo, mergedIntervals, segmentIntervals=segIntervals, allowAlignment=args.cfg)

    catMap = None
    if args.supervised is False and args.initTransProbs is not None:
        catMap = stateNamesFromUserTrans(args.initTransProbs)
        args.numStates = len(catMap)               # (the file overrides --numStates)
    truthIntervals = None
    if args.supervised is True:
        truthIntervals = trackIO.readBedIntervals(args.trainingBed, ncol=4)      # (unmerged)
        catMap = mapStateNames(truthIntervals)
        args.numStates = len(catMap)

    seeds = [random.randint(0, 4294967294)]
    if args.seed is not None:
        seeds = [args.seed]
        random.seed(args.seed)
    # (the reference draws the other seeds up to sys.maxint, which RandomState refuses above 2^32 - 1)
    seeds += [random.randint(0, 4294967294) for _ in range(1, args.reps)]
    modelList = [trainModel(seed, trackData=trackData, catMap=catMap, userTrans=None, truthIntervals=truthIntervals,
                            args=args) for seed in seeds]

    best = bestReplicate(modelList)
    if len(modelList) > 1:
        logger.info("Selecting best replicate (%d, %s)" % (best, modelList[best].getLastLogProb()))
    logger.info("saving trained model to %s" % args.outputModel)
    modelIO.saveModel(args.outputModel, modelList[best])
    writtenCount = 0
    if args.saveAllReps is True:
        for i, repModel in enumerate(modelList):
            if i != best:                          # (best == -1, no log-probability anywhere: every replicate is written)
                modelIO.saveModel("%s.rep%d" % (args.outputModel, writtenCount), repModel)
                writtenCount += 1
    return 0


def bestReplicate(modelList):
    """Index of the model with the highest last log-probability (teHmmTrain.py:294-306); -1, the last model, when
    none has one above LOGZERO (a supervised model has None, which Python 2 orders below every number)."""
    best = (-1, LOGZERO)
    for i, model in enumerate(modelList):
        if _py2_gt(model.getLastLogProb(), best[1]):
            best = (i, model.getLastLogProb())
    return best[0]


def trainModel(randomSeed, trackData, catMap, userTrans, truthIntervals, args):
    """The whole training pipeline of one replicate (teHmmTrain.py:326-414)."""
    from .emission import IndependentMultinomialAndGaussianEmissionModel
    from .hmm import MultitrackHmm
    randGen = np.random.RandomState(randomSeed)
    randomize = args.supervised is False and args.flatEm is False      # (only Baum-Welch starts from a random model)
    emissionModel = IndependentMultinomialAndGaussianEmissionModel(
        args.numStates, trackData.getNumSymbolsPerTrack(), trackData.getTrackList(), normalizeFac=args.emFac,
        randomize=randomize, effectiveSegmentLength=args.segLen, random_state=randGen, randRange=args.emRandRange)
    if args.cfg is True:
        # teHmmTrain.py:364-374
        from .cfg import MultitrackCfg
        from .emission import PairEmissionModel
        pairEM = PairEmissionModel(emissionModel, [args.saPrior] * emissionModel.getNumStates())
        nestStates = []
        if args.pairStates is not None:
            for name in args.pairStates.split(","):
                if not catMap.has(name):
                    raise RuntimeError("--pairStates: state %s is not in the training BED" % name)
                nestStates.append(catMap.getMap(name))
        logger.info("Creating cfg model")
        model = MultitrackCfg(emissionModel, pairEM, nestStates, state_name_map=catMap)
        model.supervisedTrain(trackData, truthIntervals)
        return model
    model = MultitrackHmm(emissionModel, n_iter=args.iter, state_name_map=catMap, fixTrans=args.fixTrans,
                          fixEmission=args.fixEm, fixStart=args.fixStart, forceUserEmissions=args.forceEmProbs,
                          forceUserTrans=args.forceTransProbs, random_state=randGen, thresh=args.emThresh,
                          transMatEpsilons=args.transMatEpsilons, maxProb=args.maxProb, maxProbCut=args.maxProbCut)
    # the user's starting model
    if args.initTransProbs is not None:
        with open(args.initTransProbs) as f:
            model.applyUserTrans(f.readlines())
    if args.initEmProbs is not None:
        with open(args.initEmProbs) as f:
            model.trackList = trackData.getTrackList()     # (emissions cannot be applied without a track list)
            model.applyUserEmissions(f.readlines())
    if args.initStartProbs is not None:
        with open(args.initStartProbs) as f:
            model.applyUserStarts(f.readlines())
    model.validate()

    if args.supervised is False:
        logger.info("training via EM")
        model.train(trackData)
    else:
        logger.info("training from input bed states")
        model.supervisedTrain(trackData, truthIntervals)

    # the forced entries once more, on the final model
    if args.forceTransProbs is not None:
        with open(args.forceTransProbs) as f:
            model.applyUserTrans(f.readlines())
    if args.forceEmProbs is not None:
        with open(args.forceEmProbs) as f:
            model.applyUserEmissions(f.readlines())
    return model


def stateNamesFromUserTrans(userTransPath):
    """The state names of a transition file, numbered in the order they appear (teHmmTrain.py:418-430)."""
    from .track import CategoryMap
    catMap = CategoryMap(reserved=0)
    with open(userTransPath, "r") as f:
        for toks in _user_lines(f):
            assert len(toks) == 3
            float(toks[2])
            catMap.getMap(toks[0], update=True)
            catMap.getMap(toks[1], update=True)
    return catMap


def mapStateNames(bedIntervals):
    """State names (column 4) of the intervals to integers, in place; the map is returned (teHmmTrain.py:434-444)."""
    from .track import CategoryMap
    catMap = CategoryMap(reserved=0)
    for idx, interval in enumerate(bedIntervals):
        if len(interval) < 4 or interval[3] is None:
            raise RuntimeError("Could not read state from 4th column %s" % str(interval))
        bedIntervals[idx] = (interval[0], interval[1], interval[2], catMap.getMap(interval[3], update=True))
    return catMap


if __name__ == "__main__":
    sys.exit(main())
