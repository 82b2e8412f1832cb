"""bootstrapModel -- the reference's bin/bootstrapModel.py: write the transition and emission distributions of a
trained model as the text files train's --initTransProbs / --forceTransProbs and --initEmProbs / --forceEmProbs read,
so that a supervised model can seed (part of) an unsupervised run.

Emissions are formatted as the reference formats them: %.12e after its round-down helper (floor at steps of 12^-11),
which keeps a written row from summing above 1.  Transitions go the same way (quirk Q25): the reference writes them
with %e, and a row of seven-digit numbers can sum above 1 by more than applyUserTrans accepts, so that the reference
can refuse the --allTrans file it has just written.  The added states' --stp is written with %e as there."""
import argparse
import random
import string
import sys

import numpy as np

from .common import logger


def parseArgs(argv):
    parser = argparse.ArgumentParser(
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
        description="Create starting transition and emission distributions that be used with train using the "
        "--initTransProbs and --initEmProbs options, respectively.  The distributions will be derived by an "
        "already-trained model.")
    parser.add_argument("inputModel", help="Path of input model to use for bootstrap parameter creation")
    parser.add_argument("outTransProbs", help="File to write transition model to (for use with --initTransProbs and "
                        "--forceTransProbs)")
    parser.add_argument("outEmProbs", help="File to write emission model to (for use with --initEmProbs and "
                        "--forceEmProbs)")
    parser.add_argument("--ignore", help="comma-separated list of states to ignore from inputModel", default=None)
    parser.add_argument("--numAdd", help="Number of \"unlabeled\" states to add to the model.", default=0, type=int)
    parser.add_argument("--numTotal", help="Add unlabeled states such that output model has given number of states.  "
                        "If input model already has a greater number of states then none added", default=0, type=int)
    parser.add_argument("--stp", help="Self-transition probality assigned to added states.", default=0.9, type=float)
    parser.add_argument("--allTrans", help="By default only self-transitions are written.  Use this option to write "
                        "entire transition matrix (excluding ignroed states)", default=False, action="store_true")
    args = parser.parse_args(argv)
    if args.numAdd != 0 and args.numTotal != 0:
        raise RuntimeError("--numAdd and --numTotal mutually exclusive")
    args.ignore = set() if args.ignore is None else set(args.ignore.split(","))
    return args


def main(argv=None):
    """The command line of bin/bootstrapModel.py: inputModel outTransProbs outEmProbs [options]."""
    from . import modelIO
    from .track import CategoryMap
    args = parseArgs(sys.argv[1:] if argv is None else argv)
    logger.info("loading model %s" % args.inputModel)
    model = modelIO.loadModel(args.inputModel)
    stateMap = model.getStateNameMap()
    if stateMap is None:                           # (a name for every state)
        stateMap = CategoryMap(reserved=0)
        for i in range(model.getEmissionModel().getNumStates()):
            stateMap.getMap(str(i), update=True)
    writeTransitions(model, stateMap, args)
    writeEmissions(model, stateMap, args)
    return 0


def writeTransitions(hmm, stateMap, args):
    """FROM TO PROB lines: the self transitions, or with --allTrans the whole matrix, without the ignored states; then
    the added "Unlabeled" states with their self transition (bootstrapModel.py:90-128)."""
    tranProbs = hmm.getTransitionProbs()
    numStates = len(tranProbs)
    assert len(stateMap) == numStates
    count = 0
    with open(args.outTransProbs, "w") as tfile:
        for fromStateNo in range(numStates):
            fromName = stateMap.getMapBack(fromStateNo)
            assert fromName is not None
            if fromName in args.ignore:
                continue
            count += 1
            for toStateNo in range(numStates):
                toName = stateMap.getMapBack(toStateNo)
                assert toName is not None
                if toName not in args.ignore and (args.allTrans is True or fromStateNo == toStateNo):
                    # (quirk Q25: not the reference's "%e", whose seven digits let a row sum above 1)
                    tfile.write("%s\t%s\t%.12e\n" % (fromName, toName, roundDown(tranProbs[fromStateNo, toStateNo])))
        numAdd = args.numAdd
        if args.numTotal > count:
            numAdd = args.numTotal - count
        for i in range(numAdd):
            name = "Unlabeled%d" % i
            if stateMap.has(name) is True:
                name += "_%s" % "".join(random.choice(string.ascii_uppercase + string.digits) for _ in range(5))
            assert stateMap.has(name) is False
            tfile.write("%s\t%s\t%e\n" % (name, name, args.stp))


def roundDown(f, d=12):
    """The reference's rd(): floor at steps of 12^-(d - 1), so that no written row sums above 1."""
    x = np.power(12., d - 1.)
    return np.floor(x * f) / float(x)


def writeEmissions(hmm, stateMap, args):
    """STATE TRACK SYMBOL PROB lines (gaussian tracks: STATE TRACK MEAN STDEV; binary tracks: the probability of
    symbol "1" only) -- bootstrapModel.py:131-175."""
    em = hmm.getEmissionModel()
    emProbs = np.exp(em.getLogProbs())
    trackList = hmm.getTrackList()
    assert len(trackList) > 0
    numStates = len(emProbs[0])
    assert len(stateMap) == numStates
    assert len(trackList) == len(emProbs)
    with open(args.outEmProbs, "w") as efile:
        for stateNo in range(numStates):
            stateName = stateMap.getMapBack(stateNo)
            if stateName in args.ignore:
                continue
            for track in trackList:
                trackName, trackNo = track.getName(), track.getNumber()
                if track.getDist() == "gaussian":
                    mean, stdev = em.getGaussianParams(trackNo, stateNo)
                    efile.write("%s\t%s\t%.12e\t%.12e\n" % (stateName, trackName, mean, stdev))
                elif track.getDist() == "binary":
                    efile.write("%s\t%s\t%s\t%.12e\n" % (stateName, trackName, "1",
                                                         roundDown(emProbs[trackNo][stateNo][2])))
                else:
                    for symbolName, symbolId in track.getValueMap().fwd.items():
                        efile.write("%s\t%s\t%s\t%.12e\n" % (stateName, trackName, symbolName,
                                                             roundDown(emProbs[trackNo][stateNo][symbolId])))


if __name__ == "__main__":
    sys.exit(main())
