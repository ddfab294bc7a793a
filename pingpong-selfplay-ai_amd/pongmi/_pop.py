"""What the population classes share (DQNPopulation, pongmi.dqn_pop; PopulationRollout, pongmi.rollout): the
one-value-or-n-values rule of their per-member arguments, and the life cycle of the library handle behind a
device table (csrc/pm_pop.h). A population owns its record, its checks and its decision when the table changed.
"""
import ctypes

import numpy as np
import torch

from ._lib import check

_SEQ = (list, tuple, np.ndarray, torch.Tensor)


def per_member(who, name, v, n, pair=False):
    """`v` as a list of n values: one value for all members, or a sequence of n. pair: a value is itself a pair
    (betas), so one pair stands for all members and a sequence of n pairs for one each."""
    if pair:
        seq = isinstance(v, _SEQ) and len(v) > 0 and isinstance(v[0], _SEQ)
        if not seq and not (isinstance(v, _SEQ) and len(v) == 2):
            raise ValueError(f"{who}: {name} {v!r} (a pair, or a sequence of n pairs)")
    else:
        seq = isinstance(v, _SEQ)
    if not seq:
        return [v] * n
    if len(v) != n:
        raise ValueError(f"{who}: {name} has {len(v)} values for {n} members")
    return [x.item() if isinstance(x, (np.generic, torch.Tensor)) and not pair else x for x in v]


class TableHandle:
    """Base of a class that keeps a device table in the library behind `self.lib`. `_handle` is the library's handle,
    None until the first _table call; `_entry` names its entry points (`_entry`_create, _rebind, _destroy)."""
    _entry = None  # "pm_dqn_pop", "pm_rollout_pop"
    _handle = None

    def _table(self, changed, create_args, rebind_args):
        """First use: `_entry`_create(*create_args, &handle). Later, if `changed`: `_entry`_rebind(handle, *rebind_args)."""
        if self._handle is None:
            h = ctypes.c_void_p()
            check(getattr(self.lib, self._entry + "_create")(*create_args, ctypes.byref(h)), self._entry + "_create")
            self._handle = h
        elif changed:
            check(getattr(self.lib, self._entry + "_rebind")(self._handle, *rebind_args), self._entry + "_rebind")

    def __del__(self):
        try:
            if self._handle is not None:
                getattr(self.lib, self._entry + "_destroy")(self._handle)
                self._handle = None
        except Exception:
            pass
