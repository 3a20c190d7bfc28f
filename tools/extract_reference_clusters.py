"""Extract the cluster centres of the reference's two shipped clustering results into tests/golden/representative_days_reference.npz.

    python tools/extract_reference_clusters.py <root of a DISPATCHES checkout>

Reads two DATA files of dispatches/workflow/train_market_surrogates/dynamic/ (JSON written by tslearn's to_json; no program text is read
or copied) and keeps `model_params.cluster_centers_` only:

  RE_case_study/RE_224years_20clusters_OD.json            [20, 2, 24]  (cluster, channel, hour): dispatch and wind capacity factor
        -> re_centers [20, 48], the two channels one after the other - the feature order of representative_days.py
  NE_case_study/NE_result_192years_30clusters_OD.json     [30, 24, 1]  (cluster, hour, channel)
        -> ne_centers [30, 24]

A few KB.  Nothing of the checkout is read at test or bench time: the tests see this file alone."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DYNAMIC = os.path.join("dispatches", "workflow", "train_market_surrogates", "dynamic")


def main(reference_root):
    centers = lambda *path: np.asarray(json.load(open(os.path.join(reference_root, DYNAMIC, *path)))["model_params"]["cluster_centers_"], np.float64)
    re, ne = centers("RE_case_study", "RE_224years_20clusters_OD.json"), centers("NE_case_study", "NE_result_192years_30clusters_OD.json")
    assert re.shape == (20, 2, 24) and ne.shape == (30, 24, 1), (re.shape, ne.shape)
    out = os.path.join(HERE, "tests", "golden", "representative_days_reference.npz")
    np.savez_compressed(out, re_centers=re.reshape(20, 48), ne_centers=ne.reshape(30, 24))
    print(f"{out}: re_centers [20, 48], ne_centers [30, 24], {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
