"""Strict full-message census of the reference v1 configs: every
trainer_config_helpers/tests/configs/*.py of a reference tree is run unmodified
through parse_config and compared with its protostr/*.protostr, field by field
(proto2 semantics: an empty repeated field is absent; floats to 1e-6 relative).
Prints the exact count and the first diffs of each config.

usage: python tools/v1_census.py CONFIGS_DIR [config names...]"""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd.trainer_config_helpers as tch  # noqa: E402
from paddle_amd.trainer_config_helpers import config_proto as cp  # noqa: E402


def _diff(a, b, path=""):
    out = []
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a:
                out.append(f"{path}/{k} missing")
            elif k not in b:
                out.append(f"{path}/{k} extra")
            else:
                out += _diff(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, list) and isinstance(b, list):
        if len(a) != len(b):
            out.append(f"{path} len {len(a)} vs {len(b)}")
        for i, (x, y) in enumerate(zip(a, b)):
            out += _diff(x, y, f"{path}[{i}]")
    elif isinstance(a, float) or isinstance(b, float):
        try:
            if abs(float(a) - float(b)) > 1e-6 * max(1.0, abs(float(b))):
                out.append(f"{path} {a!r} vs {b!r}")
        except (TypeError, ValueError):
            out.append(f"{path} {a!r} vs {b!r}")
    elif a != b:
        out.append(f"{path} {a!r} vs {b!r}")
    return out


def main(argv):
    if not argv or not os.path.isdir(argv[0]):
        print(__doc__)
        return 2
    ref, only = argv[0], argv[1:]
    ex, bad = [], {}
    for f in sorted(glob.glob(os.path.join(ref, "*.py"))):
        n = os.path.basename(f)[:-3]
        if only and n not in only:
            continue
        pp = os.path.join(ref, "protostr", n + ".protostr")
        if not os.path.exists(pp):
            continue
        txt = open(pp).read()
        whole = txt.lstrip().startswith("model_config")
        exp = cp.from_text("TrainerConfig" if whole else "ModelConfig", txt, strict=True)
        try:
            c = tch.parse_config(f)
            got = c.trainer_config() if whole else c.model_config()
            d = _diff(got, exp)
            if not d:
                ex.append(n)
            else:
                bad[n] = (len(d), d[:6])
        except Exception as e:  # noqa: BLE001 -- the census records every failure
            bad[n] = ("ERR", repr(e)[:150])
    print("strict exact:", len(ex))
    for k, v in bad.items():
        print(k, v)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
