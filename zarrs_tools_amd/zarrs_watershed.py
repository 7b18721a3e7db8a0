"""zarrs_watershed — the marker-controlled watershed of a Zarr V3 array on the GPU (an extension:
the reference has no such tool).

    zarrs_watershed [--device D] [--threads N] RELIEF SEEDS OUT [--connectivity C] [--descending]
                    [--foreground-only] [--skip-empty-chunks] [reencoding args]

Every non-zero element of SEEDS (an integer array of RELIEF's shape, any chunk grid and codecs) is
a label; OUT gets, for every element of the domain, the label of the seed that reaches it over the
lowest pass of RELIEF (--descending: the highest, which floods a distance map from its maxima), 0
where no seed reaches. --foreground-only keeps the flood inside the non-zero elements of RELIEF.
OUT has the seeds' data type and fill value 0; the reencoding arguments are zarrs_filter's
(-c/--chunk-shape, -s/--shard-shape, the codec arguments, ...). The step is store.watershed.

A separate tool and not a zarrs_filter subcommand: the table of step kinds is pinned name by name
by its tests, and a record for this step is a follow-up of its own (Open).
"""
from __future__ import annotations

import argparse
import sys

from . import _abi
from .zarrs_filter import _add_reencode_args, _reencode_of, encoding_of


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="zarrs_watershed", description="Grow the labels of a seeds array over a relief "
        "array: the marker-controlled watershed, on the GPU.")
    ap.add_argument("--device", type=int, default=0, help="The GPU the watershed runs on.")
    ap.add_argument("--threads", type=int, default=0,
                    help="Host threads of the codecs (0: the store's default).")
    ap.add_argument("relief", help="The path to the relief zarr array.")
    ap.add_argument("seeds", help="The path to the seeds zarr array (an integer type).")
    ap.add_argument("output", help="The path to the output zarr array.")
    ap.add_argument("--connectivity", type=int, default=1,
                    help="Neighbours differ on at most this many axes (1 .. rank).")
    ap.add_argument("--descending", action="store_true",
                    help="Flood from the maxima of the relief instead of its minima.")
    ap.add_argument("--foreground-only", action="store_true",
                    help="Label only the non-zero elements of the relief; never cross the rest.")
    _add_reencode_args(ap)
    return ap


def step_of(a) -> dict:
    """The parsed arguments as the keyword arguments of store.watershed."""
    return {"input_path": a.relief, "seeds_path": a.seeds, "output_path": a.output,
            "connectivity": a.connectivity, "descending": bool(a.descending),
            "foreground_only": bool(a.foreground_only), "data_type": a.data_type,
            "device": a.device, "nthreads": a.threads, "encoding": encoding_of(_reencode_of(a))}


def run(a, log=print) -> dict:
    from . import store as S
    kw = step_of(a)
    store_all_before = S.store_empty_chunks()
    if a.filter_skip_empty_chunks:
        S.set_store_empty_chunks(False)
    try:
        st = S.watershed(**kw)
    finally:
        S.set_store_empty_chunks(store_all_before)
    out = S.open_array(a.output)
    log(f"watershed connectivity={kw['connectivity']} descending={kw['descending']} "
        f"foreground_only={kw['foreground_only']} {a.relief} seeds {a.seeds} -> {a.output}")
    log(f"   {st['rounds'][0]} pass rounds, {st['rounds'][1]} distance rounds, "
        f"{st['rounds'][2]} jumps")
    log(f"   -> {out.data_type} {list(out.shape)} in {st['wall_s']:.2f}s "
        f"(rw:{st['decode_s']:.2f}/{st['encode_s']:.2f} p:{st['kernel_s']:.3f})")
    return st


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    try:
        run(a)
    except _abi.FilterError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
