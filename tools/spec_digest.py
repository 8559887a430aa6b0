#!/usr/bin/env python
"""What the host side of the specialised kernel produces, as digests: for every model fixture of tests/golden and every TD_SPEC_*
variant below, one sha256 over the generated source, the eight bound tables (with n_seg, sfx_first, z) and the eight impulse-response
tables (with the restart flag) at lcap 40, 258 and 1026.  Run against two builds (TD_LIB_PATH names the library) the two outputs are
equal exactly when td_spec_plan.cpp / td_jit.hip / td_spec_bounds.cpp generate the same kernels and tables.   usage: tools/spec_digest.py out.json"""
import glob
import hashlib
import json
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from tagdust_amd import lib as tdlib

VARIANTS = {
    "defaults": {}, "prune0": {"TD_SPEC_PRUNE": "0"}, "sfx0": {"TD_SPEC_PRUNE_SFX": "0"}, "restart1": {"TD_SPEC_RESTART": "1"},
    "firstseg1": {"TD_SPEC_FIRSTSEG": "1"}, "rtmin3": {"TD_SPEC_RT_MIN": "3"}, "groupcols": {"TD_SPEC_GROUPCOLS": "12", "TD_SPEC_GROUPCOLS_FWD": "8"},
    "triesh1": {"TD_SPEC_TRIE_SH": "1"}, "block256": {"TD_SPEC_BLOCK": "256", "TD_SPEC_MINWAVES": "2"}, "lsum_oob0": {"TD_SPEC_LSUM_OOB": "0"},
    "profile": {"TD_SPEC_PROFILE": "1", "TD_SPEC_PRUNE_STATS": "1"},
}
for k in [k for k in os.environ if k.startswith("TD_SPEC_") and k != "TD_SPEC_CACHE_DIR"]:
    del os.environ[k]
golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
out = {}
for path in sorted(glob.glob(os.path.join(golden, "*.npz"))):
    z = np.load(path)
    md = {k: z[k] for k in z.files}
    if "trans" not in md:
        continue
    for vname, env in VARIANTS.items():
        os.environ.update(env)
        h = hashlib.sha256(tdlib.spec_source(md).encode())
        for lcap in (40, 258, 1026):
            info = tdlib.spec_prune_info(md, lcap)
            h.update(struct.pack("<iif", info["n_seg"], info["sfx_first"], info["z"]))
            for t in ("fb", "bwb", "wa", "wb", "fbs", "bws", "wc", "wd"):
                h.update(info[t].tobytes())
            gq, gf, restart = tdlib.spec_restart_info(md, lcap)
            h.update(gq.tobytes() + gf.tobytes() + struct.pack("<i", restart))
        out[os.path.splitext(os.path.basename(path))[0] + "/" + vname] = h.hexdigest()
        for k in env:
            del os.environ[k]
with open(sys.argv[1], "w") as f:
    f.write(json.dumps(out, indent=0, sort_keys=True) + "\n")
print(len(out), "digests ->", sys.argv[1])
