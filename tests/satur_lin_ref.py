"""numpy restatement of SATUR's LDPHYLIN branch (satur.F90:106-123) and of its two partial derivatives, for the tests of the
differentiated SATUR (host and GPU).  Plain IEEE arithmetic in the reference's operation order."""
from __future__ import annotations

import numpy as np


def satur_numpy(prm, pap: np.ndarray, t: np.ndarray):
    """(qsat, zqs before the ZQMAX clamp) on float64 arrays"""
    pap, t = np.asarray(pap, dtype=np.float64), np.asarray(t, dtype=np.float64)
    xa = (np.maximum(prm.rtice, np.minimum(prm.rtwat, t)) - prm.rtice) * prm.rtwat_rtice_r
    zalfa = np.minimum(1.0, xa * xa)
    fl = prm.r2es * np.exp(prm.r3les * (t - prm.rtt) / (t - prm.r4les))
    fi = prm.r2es * np.exp(prm.r3ies * (t - prm.rtt) / (t - prm.r4ies))
    zqs0 = (zalfa * fl + (1.0 - zalfa) * fi) / pap
    zqs = np.minimum(zqs0, 0.5)
    return zqs / (1.0 - prm.retv * zqs), zqs0


def satur_partials_numpy(prm, pap: np.ndarray, t: np.ndarray):
    """(dqs/dpap, dqs/dt, clamped mask): exactly 0 where the clamp acts; one-sided values at the kinks as the library documents"""
    pap, t = np.asarray(pap, dtype=np.float64), np.asarray(t, dtype=np.float64)
    xa = (np.maximum(prm.rtice, np.minimum(prm.rtwat, t)) - prm.rtice) * prm.rtwat_rtice_r
    zalfa = np.minimum(1.0, xa * xa)
    dzalfa = np.where((t > prm.rtice) & (t < prm.rtwat), 2.0 * xa * prm.rtwat_rtice_r, 0.0)
    fl = prm.r2es * np.exp(prm.r3les * (t - prm.rtt) / (t - prm.r4les))
    fi = prm.r2es * np.exp(prm.r3ies * (t - prm.rtt) / (t - prm.r4ies))
    dfl = fl * prm.r3les * (prm.rtt - prm.r4les) / (t - prm.r4les) ** 2
    dfi = fi * prm.r3ies * (prm.rtt - prm.r4ies) / (t - prm.r4ies) ** 2
    dfoeew = dzalfa * (fl - fi) + zalfa * dfl + (1.0 - zalfa) * dfi
    zqs0 = (zalfa * fl + (1.0 - zalfa) * fi) / pap
    clamped = zqs0 > 0.5
    zqs = np.minimum(zqs0, 0.5)
    zcor = 1.0 / (1.0 - prm.retv * zqs)
    dt = np.where(clamped, 0.0, zcor * zcor * dfoeew / pap)
    dp = np.where(clamped, 0.0, -zcor * zcor * zqs / pap)
    return dp, dt, clamped
