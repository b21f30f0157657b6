"""Writes tests/golden/noise_budget.json: the reference's Decryptor::invariantNoiseBudget (oracle/_ref, where the reference was built) on
ciphertexts that every test can reproduce WITHOUT the reference.  A record is a recipe -- parameter set, key seed, encryptor seed, a sequence of
operations (tests/noise_cases.py Setup.run_sequence: this library's host KeyGenerator / Encryptor and oracle.Oracle.eval, all deterministic) --
plus the budget the reference returned for the resulting ciphertext.  Recorded results only.

    python tests/golden/gen_noise_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import noise_cases as NC  # noqa: E402
from oracle import ref as R  # noqa: E402


def main():
    assert R.available(), "oracle/_ref is missing: build the reference driver first (make -C oracle ref)"
    records = []
    for name, cfg in NC.CONFIGS.items():
        S = NC.Setup(cfg, relin=True, host_only=True)
        ref = NC.make_ref(S)
        for seq in NC.SEQUENCES:
            ct = S.run_sequence(seq)
            budget = ref.decrypt(R.Ct(ct.data, False, 1.0, ct.correction_factor))[1]
            records.append(dict(config=name, key_seed=list(NC.KEY_SEED), enc_seed=list(NC.ENC_SEED), sequence=seq, size=ct.size, limbs=ct.limbs, budget=budget))
            print(records[-1], flush=True)
    with open(NC.GOLDEN, "w") as f:
        json.dump(dict(source="Decryptor::invariantNoiseBudget of the reference's CPU build (src/decryptor.cpp:373-441)", records=records), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
