"""The conditions on tests/golden/cov_edges.npz, shared by oracle/gen_golden.py (which asserts them when it writes the file,
on the reference alone) and tests/test_gpu_cov_edges.py (which asserts them again on the committed file)."""
import numpy as np

KIND_SYNTH, KIND_ADV, KIND_TAIL, KIND_EDGE, KIND_TINY = 0, 1, 2, 3, 4
MIN_RETURN = 0.90                            # share of a set's reads on which the reference returns (status 0)
MIN_DIFFER = 0.50                            # share of (t, l, cout) whose result changes across a threshold


def class_floor(h, d):
    """Least share of each of E, H, D, R among the labelled bases of a set's generator reads."""
    return 0.01 if (h, d) == (1, 2) else 0.03


def structure(st, iv, rv, lab):
    """What of a read's result changes only with a DECISION, not with every count: status, interval boundaries, reliability,
    classes, and which of the records' error probabilities were ever computed (-inf: never; a wall the table decides has
    none, wall.c:672-675).  The counts and the finite doubles, which differ between any two profiles, are left out."""
    return (st, iv["b"].tobytes(), iv["e"].tobytes(), iv["is_rel"].tobytes(), rv["b"].tobytes(), lab,
            b"".join(np.isinf(iv[f]).tobytes() for f in ("pe", "peo_b", "peo_e")))


def edge_shares(g, si, intvl_dtype):
    """For set si of cov_edges.npz (g: its arrays): the share of reads that return, the class shares over the labelled
    bases of the generator reads, the share of the threshold-edge (t, l, cout) for which some threshold c of the triple
    (SELF or OTHERS, INIT or FINAL) has the reads with cin = c-1 and cin = c+1 end differently, and their number."""
    idx = np.nonzero(g["set"] == si)[0]
    K = int(g["psets"][si][0])
    ret = float((g["status"][idx] == 0).mean())
    lo, io, ro = g["labels_off"], g["intvl_off"], g["rintvl_off"]
    gen = [i for i in idx if g["kind"][i] in (KIND_SYNTH, KIND_ADV, KIND_TAIL) and g["status"][i] == 0]
    lab = np.concatenate([g["labels"][lo[i] + K - 1:lo[i + 1]] for i in gen])
    cls = {c: float((lab == ord(c)).mean()) for c in "EHDR"}
    iv_all, rv_all = g["intvl"].view(intvl_dtype), g["rintvl"].view(intvl_dtype)
    res, thr = {}, {}
    for i in idx:
        if g["kind"][i] == KIND_EDGE:
            t, l, cout, e, cin, c0, c1, _ = (int(x) for x in g["edge_meta"][g["edge_row"][i]])
            thr[(t, l, cout, e)] = {c0, c1}
            res[(t, l, cout, e, cin)] = structure(int(g["status"][i]), iv_all[io[i]:io[i + 1]], rv_all[ro[i]:ro[i + 1]],
                                                  g["labels"][lo[i]:lo[i + 1]].tobytes())
    triples = sorted(set(k[:3] for k in thr))
    differ = 0
    for tri in triples:
        differ += any(res.get(tri + (e, c - 1)) is not None and res.get(tri + (e, c + 1)) is not None
                      and res[tri + (e, c - 1)] != res[tri + (e, c + 1)] for e in (0, 1) for c in thr.get(tri + (e,), ()))
    return ret, cls, differ / max(1, len(triples)), len(triples)
