"""The sweep of the scoring tail's hyper-parameters (Hybridgl_main.py:57-63: r, alpha, k1, k2): the parts that need no GPU.

    parse_sweep_spec      the --sweep SPEC of hybridgl_amd.main -> the list of configurations
    pack_rows / unpack_rows   [C, n, 6] per-configuration rows + [n, 5] ceiling rows <-> the [m, 6] rows dist.gather_rows moves
    sweep_metrics_from_rows   the report per configuration, the ceiling's and the best configuration

The device side is ops.score_group_sweep (hgl_score_group_sweep); HybridGLPipeline(sweep=...) drives it.
"""
import itertools

import numpy as np

from .dist import ROW_FIELDS, metrics_from_rows

AXES = ("r", "alpha", "k1", "k2")
ENDPOINT_EPS = 1e-9


def _axis_values(name, text):
    """one axis: `v,v,...` or `lo:hi:step` (hi included when a step reaches it within ENDPOINT_EPS); k1 / k2 are integers"""
    integer = name in ("k1", "k2")

    def number(tok):
        tok = tok.strip()
        try:
            return int(tok) if integer else float(tok)
        except ValueError:
            raise ValueError(f"--sweep: axis {name}: {tok!r} is not {'an integer' if integer else 'a number'}") from None

    if ":" in text:
        parts = text.split(":")
        if len(parts) != 3:
            raise ValueError(f"--sweep: axis {name}: a range is lo:hi:step, got {text!r}")
        lo, hi, step = (number(p) for p in parts)
        if not step > 0 or hi < lo:
            raise ValueError(f"--sweep: axis {name}: a range needs step > 0 and hi >= lo, got {text!r}")
        vals, i = [], 0
        while lo + i * step <= hi + ENDPOINT_EPS:
            vals.append(lo + i * step)      # (not a running sum: no error builds up over the steps)
            i += 1
        return vals
    return [number(tok) for tok in text.split(",")]


def parse_sweep_spec(spec, r, alpha, k1, k2):
    """`r=0.3,0.5,0.7;alpha=0:1:0.1;k1=3;k2=6` -> [(r, alpha, k1, k2), ...].  Axes are separated by `;`, an axis is a value
    list or lo:hi:step; an axis that is left out keeps the run's value (the arguments).  The result is the cartesian product
    in the fixed order r (slowest), alpha, k1, k2 (fastest), each axis in the order it was written -- whatever the order of
    the axes in the spec.  ValueError for anything else (unknown or repeated axis, empty axis, not a number, k < 1)."""
    axes = {}
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("--sweep: empty spec")
    for part in spec.split(";"):
        if not part.strip():
            continue
        if "=" not in part:
            raise ValueError(f"--sweep: expected axis=values, got {part!r}")
        name, text = (t.strip() for t in part.split("=", 1))
        if name not in AXES:
            raise ValueError(f"--sweep: unknown axis {name!r} (the axes are {', '.join(AXES)})")
        if name in axes:
            raise ValueError(f"--sweep: axis {name} given twice")
        if not text:
            raise ValueError(f"--sweep: axis {name} is empty")
        axes[name] = _axis_values(name, text)
    if not axes:
        raise ValueError("--sweep: empty spec")
    default = dict(r=float(r), alpha=float(alpha), k1=int(k1), k2=int(k2))
    lists = [axes.get(n, [default[n]]) for n in AXES]
    if any(k < 1 for k in lists[2] + lists[3]):
        raise ValueError("--sweep: k1 and k2 start at 1")
    return [(float(a), float(b), int(c), int(d)) for a, b, c, d in itertools.product(*lists)]


def pack_rows(rows, ceiling):
    """rows [C, n, 6] (ROW_FIELDS per configuration) and ceiling [n, 5] (position, sentence, proposal, I, U) -> [n (C + 1), 6]
    int64: sentence-major, the sentence's C configuration rows followed by its ceiling as (position, sentence, I, U, I, U), so
    that ranks' blocks can simply be concatenated (dist.gather_rows)"""
    rows = np.asarray(rows, dtype=np.int64)
    ceiling = np.asarray(ceiling, dtype=np.int64).reshape(-1, 5)
    C, n = rows.shape[0], rows.shape[1]
    assert rows.shape == (C, n, len(ROW_FIELDS)) and ceiling.shape[0] == n
    out = np.empty((n, C + 1, len(ROW_FIELDS)), dtype=np.int64)
    out[:, :C] = rows.transpose(1, 0, 2)
    out[:, C, 0:2] = ceiling[:, 0:2]
    out[:, C, 2:4] = ceiling[:, 3:5]
    out[:, C, 4:6] = ceiling[:, 3:5]
    return out.reshape(-1, len(ROW_FIELDS))


def unpack_rows(packed, C):
    """the inverse of pack_rows up to the ceiling's proposal index: (rows [C, n, 6], ceiling rows [n, 6] as
    (position, sentence, I, U, I, U))"""
    packed = np.asarray(packed, dtype=np.int64).reshape(-1, C + 1, len(ROW_FIELDS))
    return np.ascontiguousarray(packed[:, :C].transpose(1, 0, 2)), np.ascontiguousarray(packed[:, C])


def sweep_metrics_from_rows(rows, ceiling6, configs=None):
    """{"configs": [metrics_from_rows(rows[c]) (+ r, alpha, k1, k2 when `configs` is given) per configuration], "ceiling":
    {oIoU, mIoU, cum: [I, U], n_sentences} of the best proposal per sentence, "best": the index of the configuration with
    the largest oIoU_final (the first of equals; None without configurations)}"""
    per = []
    for c in range(len(rows)):
        m = metrics_from_rows(rows[c])
        if configs is not None:
            m.update(dict(zip(("r", "alpha", "k1", "k2"), configs[c])))
        per.append(m)
    cm = metrics_from_rows(ceiling6)
    best = None
    for c, m in enumerate(per):
        if best is None or m["oIoU_final"] > per[best]["oIoU_final"]:
            best = c
    return {"configs": per,
            "ceiling": {"oIoU": cm["oIoU"], "mIoU": cm["mIoU"], "cum": cm["cum"][:2], "n_sentences": cm["n_sentences"]},
            "best": best}
