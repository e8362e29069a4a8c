"""The packed sampler weights, pinned by recorded digests (tests/golden/packed_weight_digests.json).

A load (PolicyBank.load_trainable, CommanderNet.set_weights) and a device refresh go through ONE packer, so comparing one with the other
proves nothing about the bytes.  The fixture holds, for every case of the byte-identity tests of test_gpu_weight_refresh.py, the SHA-256
and length of every packed part as the commit named in it wrote them (its host-side packer, since deleted), and a SHA-256 of the input
weights, which tells a drift of the weight generator (numpy) apart from one of the packer.

    python tests/packed_weight_digests.py --record --parent-commit HASH [--out FILE]   # on an MI355X, HH_WORLD_LIB = that commit's library
    python tests/packed_weight_digests.py --check                                     # the library in use against the fixture
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "packed_weight_digests.json")
POLICY_CASES = [(mode, seeds, tie) for mode in ("fight", "escape") for seeds in ((3, 11), (17, 5)) for tie in (True, False)]
COMMANDER_CASES = [(2, 9), (9, 4)]
POLICY_PARTS, COMMANDER_PARTS = (0, 1, 2, 3, 4), (0, 1)


def policy_case(mode, seeds, tie):
    return f"{mode}-{seeds[0]}-{seeds[1]}-{'tied' if tie else 'untied'}"


def commander_case(seeds):
    return f"{seeds[0]}-{seeds[1]}"


def policy_weights(mode, seeds, tie):
    """(kinds, actor dicts, critic dicts) of a case: the second seed, the edge values with seeds (17, 5)"""
    from test_gpu_weight_refresh import _dicts
    return _dicts(mode, seeds[1], tie, edges=seeds == (17, 5))


def commander_weights(seeds):
    from hhmarl_2d_amd import commander as CM
    sd = CM.random_weights(seeds[1])
    if seeds == (9, 4):
        sd["rnn_act.bias_ih_l0"][:4] = np.array([1e-39, 3.0, -0.0, 2.0 ** -25], np.float32)
        sd["rnn_act.bias_hh_l0"][:4] = np.array([-1e-39, 2.0 ** -24, 0.0, 1e-7], np.float32)
        sd["shared_layer._model.0.weight"][7, 295:305] = 6.1e-5
    return sd


def weights_digest(dicts):
    """SHA-256 of the dicts' float32 arrays, concatenated in key order"""
    h = hashlib.sha256()
    for d in dicts:
        for v in d.values():
            h.update(np.ascontiguousarray(v, dtype=np.float32).tobytes())
    return h.hexdigest()


def digest(t):
    """a packed part (uint8 CUDA tensor) -> {"sha256", "bytes"}; waits for the current stream"""
    b = t.cpu().numpy().tobytes()
    return {"sha256": hashlib.sha256(b).hexdigest(), "bytes": len(b)}


def policy_digests(bank, slots=(0, 1)):
    return {f"{s}/{p}": digest(bank.packed(s, p)) for s in slots for p in POLICY_PARTS}


def commander_digests(net):
    return {str(p): digest(net.packed(p)) for p in COMMANDER_PARTS}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def _measure():
    """every case loaded into a fresh bank / commander by the library in use"""
    import torch
    from hhmarl_2d_amd import commander as CM
    from hhmarl_2d_amd.pilots import PolicyBank
    dev = torch.device("cuda", 0)
    out = {"policy": {}, "commander": {}}
    for case in POLICY_CASES:
        kinds, sds, csds = policy_weights(*case)
        bank = PolicyBank(dev, 64)
        for slot in (0, 1):
            bank.load_trainable(slot, kinds[slot], sds[slot], csds[slot])
        out["policy"][policy_case(*case)] = {"weights_sha256": weights_digest(sds + csds), "parts": policy_digests(bank)}
    for seeds in COMMANDER_CASES:
        sd = commander_weights(seeds)
        net = CM.CommanderNet(0, 96).set_weights(sd)
        out["commander"][commander_case(seeds)] = {"weights_sha256": weights_digest([sd]), "parts": commander_digests(net)}
    return out


def main(argv):
    sys.path.insert(0, os.path.dirname(HERE))
    if "--record" in argv:
        commit = argv[argv.index("--parent-commit") + 1]
        path = argv[argv.index("--out") + 1] if "--out" in argv else FIXTURE
        doc = {"parent_commit": commit, "numpy": np.__version__, **_measure()}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(doc['policy'])} policy and {len(doc['commander'])} commander cases -> {path}")
        return 0
    if "--check" in argv:
        want, got = load(), _measure()
        bad = []
        for grp in ("policy", "commander"):
            for case, rec in got[grp].items():
                if rec["weights_sha256"] != want[grp][case]["weights_sha256"]:
                    bad.append((grp, case, "the input weights (the generator, not the packer)"))
                bad += [(grp, case, "part " + k) for k, v in rec["parts"].items() if v != want[grp][case]["parts"][k]]
        for b in bad:
            print("differs:", *b)
        print(f"{'FAILED' if bad else 'ok'}: {len(got['policy'])} policy and {len(got['commander'])} commander cases against "
              f"{want['parent_commit'][:12]} (numpy {want['numpy']} then, {np.__version__} now)")
        return 1 if bad else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
