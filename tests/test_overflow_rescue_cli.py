"""CPU: --on_overflow on the command line of hybridgl_amd.main, and what it excludes."""
import argparse

import pytest


def flags(**kw):
    base = dict(save_proposals="", proposals_dir="", real=True, prepare=False, on_overflow="raise")
    base.update(kw)
    return argparse.Namespace(**base)


def test_save_proposals_and_rescue_exclude_each_other():
    """a recorder's files are no part of the loop's roll-back: the store would keep what a rescue has rejected"""
    from hybridgl_amd.main import check_proposal_flags
    with pytest.raises(SystemExit, match="--save_proposals and --on_overflow rescue"):
        check_proposal_flags(flags(save_proposals="store", on_overflow="rescue"))
    check_proposal_flags(flags(save_proposals="store"))                          # the default mode records as before
    check_proposal_flags(flags(proposals_dir="store", on_overflow="rescue"))     # reading a store runs no SAM pass to reject
    check_proposal_flags(flags(on_overflow="rescue"))
