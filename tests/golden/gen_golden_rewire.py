#!/usr/bin/env python
"""Golden-vector generator for the rewire_attention block's two-hop densification.

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference tree through
gen_golden.py); nothing under tests/ imports it.  It loads gen_golden.py as a module for
its stand-ins, imports the reference's own

  * src/block_transformer_rewiring.py (RewireAttODEblock.add_khop_edges :65-93)

and calls that method, unbound, on a stub object that carries what it reads (num_nodes,
device, odefunc.edge_index [1,2,E], odefunc.edge_weight [1,E]) in float64.  Its lines
:68-77 are sound: W = sparse_coo(...).to_dense(), 0.5 W + 0.5 W·W, the diagonal masked.
The position list it derives next (:79-85) sorts the (row, col) columns independently and
is not recorded, and with the installed torch the method raises at :92 (it indexes with the
float tensor that :83 made of the positions), before it would leave the dense matrix in
``odefunc.edge_weight`` (:93).  The matrix is therefore taken where the method itself hands
it on: ``torch.zeros_like(edge_weights)`` (:79) is wrapped for the call and records its
argument, the masked 0.5 W + 0.5 W·W of :75-77.  Writes inputs + that matrix to tests/golden/rewire/khop_*.npz for the toy graph and
two seeded graphs (fixtures of tests/rewire_oracle.py: the prepared edge list and its fp32
rw-normalised weights, up-cast)."""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "rewire")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
import block_transformer_rewiring as ref_rw  # noqa: E402  (gen_golden put the reference on sys.path)

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import rewire_oracle as RO  # noqa: E402


def run(name):
    ei, w0, N = RO.prepared(name)
    stub = types.SimpleNamespace(num_nodes=N, device='cpu',
                                 odefunc=types.SimpleNamespace(edge_index=torch.from_numpy(ei),
                                                               edge_weight=torch.from_numpy(w0).double(),
                                                               attention_weights=None))
    seen = []
    zeros_like = torch.zeros_like

    def recording_zeros_like(t, *a, **k):
        seen.append(t)
        return zeros_like(t, *a, **k)

    torch.zeros_like = recording_zeros_like
    try:
        ref_rw.RewireAttODEblock.add_khop_edges(stub, k=2)
        complete = True
    except Exception as exc:  # :92 indexes with a float tensor; the dense matrix is formed before it
        complete = repr(exc)
    finally:
        torch.zeros_like = zeros_like
    S = stub.odefunc.edge_weight if complete is True else (seen[0] if seen else None)
    if not (torch.is_tensor(S) and S.dim() == 3 and tuple(S.shape) == (1, N, N)):
        raise SystemExit("add_khop_edges formed no dense matrix on the stub (%r)" % (complete,))
    meta = dict(name=name, N=N, E=int(ei.shape[2]), source="reference add_khop_edges :65-93 on a stub; the matrix "
                "as :79 passes it to zeros_like", method_completed=complete)
    np.savez_compressed(os.path.join(OUT_DIR, "khop_%s.npz" % name), edge_index=ei, w0=w0,
                        S=S.detach().double().numpy()[0], meta=json.dumps(meta))
    return meta


if __name__ == '__main__':
    os.makedirs(OUT_DIR, exist_ok=True)
    made = [run(n) for n in ('toy', 'short', 'dups')]
    with open(os.path.join(OUT_DIR, "MANIFEST.json"), "w") as fh:
        json.dump(made, fh, indent=1)
    print(made)
