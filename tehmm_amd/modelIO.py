"""Model (de)serialisation without pickle (the reference pickles the whole model object,
modelIO.py:17-32; unpickling a stranger's file executes code).  A model is its arrays plus a JSON
description of everything else teHmmEval / teHmmTrain read back from it: the track list with its value
maps (teHmmEval.py:149 re-encodes the evaluation data with the TRAINING symbols), the state-name map
(teHmmEval.py:297), the emission-model class with its gaussian parameters and the hmm-level flags.
One .npz, loaded with allow_pickle=False."""
import json

import numpy as np

FORMAT = "tehmm_amd.model.v2"
FORMAT_V1 = "tehmm_amd.model.v1"       # round-2 files: arrays only (no track list, value maps, flags)
KIND_HMM, KIND_CFG = "hmm", "cfg"      # the `kind` array of a v2 file (files from before it had one: an HMM)


def _load_v1(z):
    """Files written by the round-2 format: the arrays with default metadata (a multinomial emission model, no track
    list -- evaluation data must already be encoded with the training symbols)."""
    from .emission import IndependentMultinomialEmissionModel
    from .hmm import MultitrackHmm
    lp = z["log_probs"]
    eff = float(z["eff_seg_len"])
    em = IndependentMultinomialEmissionModel(lp.shape[1], [int(x) for x in z["symbols"]], fudge=float(z["fudge"]),
                                             effectiveSegmentLength=None if eff < 0 else eff)
    em.logProbs = lp.copy()
    em.normalizeFac = float(z["normalize_fac"])
    if z["gauss_params"].size:
        em.gaussParams = z["gauss_params"].copy()
    hmm = MultitrackHmm(em)
    hmm._log_transmat = z["log_transmat"].copy()
    hmm._log_startprob = z["log_startprob"].copy()
    it = int(z["iteration"])
    hmm.current_iteration = None if it < 0 else it
    return hmm


def _map_to_json(vm):
    from .track import BinaryMap, CategoryMap, IdentityValueMap
    if vm is None:
        return None
    if isinstance(vm, BinaryMap):
        # (written as a category map it came back as one without entries: every row of a binary track then read as
        # missing data in teHmmEval.  Files from before this type still load that way.)
        return {"type": "binary"}
    if isinstance(vm, IdentityValueMap):
        return {"type": "identity", "scale": vm.scale, "shift": vm.shift}
    if isinstance(vm, CategoryMap):
        def enc(key):                       # numeric tracks key on strings, categorical ones on the raw value
            return ["s", key] if isinstance(key, str) else ["r", repr(key)]
        return {"type": "category", "reserved": vm.reserved, "scale": vm.scale, "logBase": vm.logBase,
                "shift": vm.shift, "defaultVal": None if vm.defaultVal is None else enc(vm.defaultVal),
                "missingVal": int(vm.missingVal),
                "entries": [[enc(k), int(s)] for k, s in sorted(vm.fwd.items(), key=lambda kv: kv[1])]}
    raise TypeError("saveModel: value map of type %s cannot be serialised" % type(vm).__name__)


def _map_from_json(d):
    import ast
    from .track import BinaryMap, CategoryMap, IdentityValueMap
    if d is None:
        return None
    if d["type"] == "binary":
        return BinaryMap()
    if d["type"] == "identity":
        return IdentityValueMap(d["scale"], d["shift"])

    def dec(e):
        return e[1] if e[0] == "s" else ast.literal_eval(e[1])
    vm = CategoryMap(reserved=d["reserved"])
    vm.scale, vm.logBase, vm.shift = d["scale"], d["logBase"], d["shift"]
    vm.defaultVal = None if d["defaultVal"] is None else dec(d["defaultVal"])
    vm.missingVal = d["missingVal"]
    vm.fwd = {dec(k): int(s) for k, s in d["entries"]}
    vm.back = {s: k for k, s in vm.fwd.items()}
    return vm


def _track_to_json(t):
    return {"name": t.getName(), "number": int(t.getNumber()), "dist": t.getDist(),
            "valueMap": _map_to_json(t.getValueMap())}


def _common_meta(model):
    """What both model classes store beside their arrays: the emission model's flags, the track list, the state names."""
    from .emission import IndependentMultinomialAndGaussianEmissionModel
    em = model.getEmissionModel()
    tl = model.getTrackList()
    return {
        "emission_class": "gaussian" if isinstance(em, IndependentMultinomialAndGaussianEmissionModel) else "multinomial",
        "zeroAsMissingData": bool(em.zeroAsMissingData),
        "uniformMixProb": float(em.uniformMixProb),
        "randRange": list(em.randRange),
        "tracks": None if tl is None else [_track_to_json(t) for t in tl],
        "stateNameMap": _map_to_json(model.getStateNameMap()),
    }


def _emission_arrays(em):
    gp = getattr(em, "gaussParams", None)
    return dict(log_probs=em.getLogProbs(), symbols=np.asarray(em.getNumSymbolsPerTrack(), dtype=np.int64),
                normalize_fac=float(em.normalizeFac), fudge=float(em.fudge),
                eff_seg_len=np.asarray(-1.0 if em.effectiveSegmentLength is None else em.effectiveSegmentLength),
                gauss_params=np.zeros(0) if gp is None else gp)


def _save_cfg(path, cfg):
    """A MultitrackCfg: both production tables, start probabilities, pair states and logPriors next to the emission
    model; the alignment track travels with the track list."""
    cfg.validate()
    meta = _common_meta(cfg)
    tl = cfg.getTrackList()
    al = None if tl is None else tl.getAlignmentTrack()
    meta["alignmentTrack"] = None if al is None else _track_to_json(al)
    with open(path, "wb") as f:
        np.savez(f, format=np.asarray(FORMAT), kind=np.asarray(KIND_CFG), log_probs1=cfg.logProbs1,
                 log_probs2=cfg.logProbs2, log_startprob=cfg.startProbs,
                 nest_states=np.asarray(cfg.nestStates, dtype=np.int64),
                 log_priors=np.asarray(cfg.pairEmissionModel.logPriors, dtype=np.float64),
                 meta=np.asarray(json.dumps(meta)), **_emission_arrays(cfg.getEmissionModel()))


def saveModel(path, hmm):
    from .cfg import MultitrackCfg
    if isinstance(hmm, MultitrackCfg):
        return _save_cfg(path, hmm)
    hmm.validate()
    em = hmm.getEmissionModel()
    meta = _common_meta(hmm)
    meta.update({
        "hmm": {"fudge": float(hmm.fudge), "fixTrans": bool(hmm.fixTrans), "fixEmission": bool(hmm.fixEmission),
                "fixStart": bool(hmm.fixStart), "maxProb": bool(hmm.maxProb),
                "maxProbCut": hmm.maxProbCut, "transMatEpsilons": bool(hmm.transMatEpsilons),
                "algorithm": hmm._algorithm, "n_iter": int(hmm.n_iter), "thresh": float(hmm.thresh),
                "numZeroInitEdges": int(hmm.numZeroInitEdges), "numZeroInitStarts": int(hmm.numZeroInitStarts),
                "last_forward_log_prob": hmm.last_forward_log_prob,
                "last_forward_log_prob_it": int(hmm.last_forward_log_prob_it)},
    })
    force = {"trans": hmm.forceUserTrans, "emissions": hmm.forceUserEmissions, "start": hmm.forceUserStart}
    if any(v is not None for v in force.values()):
        # (optional key: the force line lists travel with the model, as they do in the reference's pickle)
        meta["forceUser"] = {k: None if v is None else [str(x) for x in v] for k, v in force.items()}
    with open(path, "wb") as f:
        np.savez(f, format=np.asarray(FORMAT), kind=np.asarray(KIND_HMM), log_transmat=hmm._log_transmat,
                 log_startprob=hmm._log_startprob,
                 iteration=np.asarray(-1 if hmm.current_iteration is None else hmm.current_iteration),
                 meta=np.asarray(json.dumps(meta)), **_emission_arrays(em))


def loadModel(path):
    from .emission import (IndependentMultinomialAndGaussianEmissionModel,
                           IndependentMultinomialEmissionModel)
    from .hmm import MultitrackHmm
    from .track import Track, TrackList
    with np.load(path, allow_pickle=False) as z:
        if str(z["format"]) == FORMAT_V1:
            return _load_v1(z)
        if str(z["format"]) != FORMAT:
            raise ValueError("loadModel: %s is not a %s file" % (path, FORMAT))
        meta = json.loads(str(z["meta"]))
        lp = z["log_probs"]
        eff = float(z["eff_seg_len"])
        symbols = [int(x) for x in z["symbols"]]
        kind = str(z["kind"]) if "kind" in z.files else KIND_HMM
        if kind not in (KIND_HMM, KIND_CFG):
            raise ValueError("loadModel: %s holds a model of unknown kind %r" % (path, kind))
        tl = None
        if meta["tracks"] is not None:
            tl = TrackList(Track(t["name"], t["number"], t["dist"], _map_from_json(t["valueMap"]))
                           for t in meta["tracks"])
            al = meta.get("alignmentTrack")
            if al is not None:
                tl.addTrack(Track(al["name"], al["number"], al["dist"], _map_from_json(al["valueMap"])),
                            allowAlignment=True)
        kw = dict(zeroAsMissingData=meta["zeroAsMissingData"], fudge=float(z["fudge"]),
                  effectiveSegmentLength=None if eff < 0 else eff, randRange=tuple(meta["randRange"]))
        if meta["emission_class"] == "gaussian":
            if tl is None:
                raise ValueError("loadModel: a gaussian emission model needs its track list")
            em = IndependentMultinomialAndGaussianEmissionModel(lp.shape[1], symbols, tl, **kw)
            em.gaussParams = z["gauss_params"].copy()
        else:
            em = IndependentMultinomialEmissionModel(lp.shape[1], symbols, **kw)
        em.uniformMixProb = float(meta["uniformMixProb"])
        em.logProbs = lp.copy()
        em.normalizeFac = float(z["normalize_fac"])
        if kind == KIND_CFG:
            from .cfg import MultitrackCfg
            from .emission import PairEmissionModel
            pairEM = PairEmissionModel(em, [None] * lp.shape[1])
            pairEM.logPriors = z["log_priors"].copy()
            cfg = MultitrackCfg(em, pairEM, [int(x) for x in z["nest_states"]],
                                state_name_map=_map_from_json(meta["stateNameMap"]))
            cfg.logProbs1, cfg.logProbs2 = z["log_probs1"].copy(), z["log_probs2"].copy()
            cfg.startProbs = z["log_startprob"].copy()
            cfg.trackList = tl
            cfg.createHelperTables()
            cfg.validate()
            return cfg
        h = meta["hmm"]
        hmm = MultitrackHmm(em, algorithm=h["algorithm"], n_iter=h["n_iter"], thresh=h["thresh"],
                            state_name_map=_map_from_json(meta["stateNameMap"]), fudge=h["fudge"],
                            fixTrans=h["fixTrans"], fixEmission=h["fixEmission"], fixStart=h["fixStart"],
                            transMatEpsilons=h["transMatEpsilons"], maxProb=h["maxProb"], maxProbCut=h["maxProbCut"])
        hmm.trackList = tl
        force = meta.get("forceUser") or {}
        hmm.forceUserTrans = force.get("trans")
        hmm.forceUserEmissions = force.get("emissions")
        hmm.forceUserStart = force.get("start")
        # (transmat_ / startprob_ are views of the log tables, hmm.py:622-666: zeros stay -1e100)
        hmm._log_transmat = z["log_transmat"].copy()
        hmm._log_startprob = z["log_startprob"].copy()
        hmm.numZeroInitEdges = h["numZeroInitEdges"]
        hmm.numZeroInitStarts = h["numZeroInitStarts"]
        hmm.last_forward_log_prob = h["last_forward_log_prob"]
        hmm.last_forward_log_prob_it = h["last_forward_log_prob_it"]
        it = int(z["iteration"])
        hmm.current_iteration = None if it < 0 else it
    hmm.validate()
    return hmm
