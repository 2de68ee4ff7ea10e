#!/usr/bin/env python3
"""Generates tests/golden/fast2d_tsdf_reference.json: found / score / pose of the REFERENCE'S OWN
FastCorrelativeScanMatcher2D (oracle/_ref, compiled unmodified) over its own TSDF2D, for a
selection of the searches of tests/fast2d_range_cases.py and every edge case there at truncation
distances 0.3 and 1.0.  Inputs are regenerated from seeds by that module and not stored; each
case names them: scene index, truncation distance, cloud index and full-submap flag, or the edge
case's name, and the threshold.  f32 / f64 values are stored as C99 hex floats.  Usage:
    python tests/golden/make_fast2d_tsdf_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

EDGE_TRUNCATIONS = (0.3, 1.0)


def selection(cases, synth, orc):
    """[(key dict, tsd, wgt, truncation, init or None, cloud, min_score)]: per (scene, T) the four
    cloud sizes, windowed and full-submap, at each kind of derived threshold."""
    out = []
    for index in range(len(cases.SCENES)):
        sc = cases.scene(synth, orc, index)
        for truncation in cases.TRUNCATIONS:
            tsd, wgt = sc.planes(truncation)
            mid, one, low = cases.tsdf_expectations(synth, orc, index, truncation)[1]
            for k, full, t in ((0, False, mid), (1, True, low), (3, False, one), (2, True, mid)):
                key = dict(kind="scene", scene=index, truncation=truncation, cloud=k,
                           full=bool(full), min_score=float(t).hex())
                out.append((key, tsd, wgt, truncation, None if full else sc.inits[k],
                            sc.clouds[k], t))
    for truncation in EDGE_TRUNCATIONS:
        for name, tsd, wgt, init, cloud, min_scores in cases.edge_cases(synth, orc, truncation):
            for t in min_scores:
                key = dict(kind=name, scene=cases.EDGE_SCENE, truncation=truncation,
                           min_score=float(t).hex())
                out.append((key, tsd, wgt, truncation, init, cloud, t))
    return out


def build():
    import fast2d_range_cases as cases
    from cartographer_amd import synth
    from oracle import pyoracle as orc
    assert orc.ref_lib() is not None, "needs oracle/_ref (make -C oracle ref)"
    results = []
    matchers = {}
    for key, tsd, wgt, truncation, init, cloud, t in selection(cases, synth, orc):
        sc = cases.scene(synth, orc, key["scene"])
        ident = (key["scene"], truncation, key["kind"])
        if ident not in matchers:
            matchers[ident] = orc.ReferenceFastCorrelativeScanMatcher2D.over_tsdf(
                tsd, wgt, cases.RES, sc.max_x, sc.max_y, truncation, cases.MAX_WEIGHT, sc.depth,
                cases.LIN, cases.ANG)
        m = matchers[ident]
        r = m.match_full_submap(cloud, t) if init is None else m.match(init, cloud, t)
        entry = dict(key, found=bool(r["found"]))
        if r["found"]:
            entry["score"] = float(r["score"]).hex()
            entry["pose"] = [float(v).hex() for v in r["pose"]]
        results.append(entry)
    return dict(source="reference FastCorrelativeScanMatcher2D over TSDF2D",
                linear_search_window=cases.LIN, angular_search_window=float(cases.ANG).hex(),
                cases=results)


if __name__ == "__main__":
    out = os.path.join(HERE, "fast2d_tsdf_reference.json")
    data = build()
    with open(out, "w") as f:                     # one case per line
        head = {k: v for k, v in data.items() if k != "cases"}
        f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": [\n')
        f.write(",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":"))
                           for c in data["cases"]))
        f.write("\n]}\n")
    print("wrote", out, os.path.getsize(out), "bytes")
