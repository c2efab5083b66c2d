// Chan's update of a running (n, mean, M2 = sum (x - mean)^2) by another one: what colstats.hip (corpus statistics) and gv.hip
// (per-utterance variances) merge their shifted float64 chunks with.  Counts travel as doubles (exact below 2^53); an empty side is
// skipped, never divided by, and two equal means leave the mean and M2 untouched (delta == 0: a constant column keeps M2 == 0.0).
#pragma once

__device__ __forceinline__ void mg_chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb;
        ma = mb;
        Ma = Mb;
        return;
    }
    const double n = na + nb;
    const double delta = mb - ma;
    ma = ma + delta * (nb / n);
    Ma = Ma + Mb + delta * delta * (na * nb / n);
    na = n;
}
