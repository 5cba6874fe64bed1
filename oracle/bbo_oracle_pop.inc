/*
 * oracle/bbo_oracle_pop.inc -- TEST INFRASTRUCTURE (included by bbo_oracle.cpp).
 *
 * CPU restatement of the DE / PSO generations and of the restart drivers:
 *   Shade   src/multivariate/de/shade.cpp:56-298
 *   Jade    src/multivariate/de/jade.cpp:64-294
 *   Apso    src/multivariate/pso/apso.cpp:48-452
 *   BiPop   src/multivariate/cma/bipop_cmaes.cpp:61-267
 *   IPop    src/multivariate/cma/ipop_cmaes.cpp:65-189
 *
 * Each population optimizer has two modes:
 *   async (default): the reference's loop, in-place replacement inside the i-loop, the
 *                    global mt19937 consumed in program order -> bit-exact vs oracle/_ref;
 *   sync:            generation-synchronous semantics with the counter-based generator,
 *                    i.e. exactly what the HIP kernels compute (DESIGN.md "sync semantics").
 */

namespace {

struct Point {
    std::vector<double> x;
    double f;
};

bool point_less(const Point &a, const Point &b) { return a.f < b.f; }

/* shade.cpp:258-275 / jade.cpp:228-245 / apso.cpp:129-145: Welford variance of the radii */
template<class It, class GetX>
bool radius_converged(It first, It last, GetX getx, int n, int np, double tol)
{
    int count = 0;
    double mean = 0., m2 = 0.;
    for (It it = first; it != last; ++it) {
        const double x = nrm2(n, getx(*it));
        count++;
        const double delta = x - mean;
        mean += delta / count;
        const double delta2 = x - mean;
        m2 += delta * delta2;
    }
    return m2 <= (np - 1) * tol * tol;
}

/* sync mode: two passes, plain 2-norms -- what the device reduction computes */
template<class It, class GetX>
bool radius_converged_sync(It first, It last, GetX getx, int n, int np, double tol)
{
    double sum = 0.;
    int count = 0;
    for (It it = first; it != last; ++it) {
        sum += std::sqrt(dot(n, getx(*it), getx(*it)));
        count++;
    }
    const double mean = sum / count;
    double m2 = 0.;
    for (It it = first; it != last; ++it) {
        const double r = std::sqrt(dot(n, getx(*it), getx(*it))) - mean;
        m2 += r * r;
    }
    return m2 <= (np - 1) * tol * tol;
}

const int SYNC_MAX_TRIES = 64;

/* ======================================================================== */
/* differential evolution: L-SHADE (variant 0) and JADE (variant 1)          */
/* ======================================================================== */
struct De {
    int variant = 0;
    /* parameters */
    int mfev = 0, npinit = 0, npmin = 4, h = 100;
    double tol = 0., pelite = 0.05, cdamp = 0.1, jsigma = 0.07;
    bool archive = true, repaircr = true;
    /* problem */
    int obj = 0, n = 0;
    std::vector<double> lower, upper, aux;
    /* state */
    int np = 0, fev = 0, k = 1, gen = 0;
    long repairs_lo = 0, repairs_up = 0;   /* coordinates repair() moved, per side (read-only) */
    double mucr = 0.5, muf = 0.5;
    std::vector<double> MCR, MF, work, SCR, SF, W;
    std::vector<std::vector<double>> arch;
    std::vector<Point> swarm;
    /* mode */
    bool sync = false;
    int rng_mode = RNG_MT;
    uint64_t seed = 0;
    int sub = 0;   /* population sub-stream */
    NormalCache Z;

    double evaluate(const double *p) { return bbo_objective_eval(obj, n, p, aux.data()); }

    void init(int obj_, int n_, const double *lo, const double *up)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        fev = 0;
        gen = 0;
        repairs_lo = repairs_up = 0;
        MCR.assign(h, 0.5);
        MF.assign(h, 0.5);
        mucr = muf = 0.5;
        work.assign(n, 0.);
        arch.clear();
        SCR.clear();
        SF.clear();
        W.clear();
        k = 1;
        np = npinit;
        swarm.clear();
        for (int i = 0; i < np; i++) {
            Point p;
            p.x.resize(n);
            for (int j = 0; j < n; j++) {
                if (rng_mode == RNG_MT) {
                    p.x[j] = mt_uniform(lower[j], upper[j]);
                } else {
                    /* sync init: u(i, j) from the INIT stream, two coordinates per call */
                    uint32_t w[4];
                    bbo_philox(seed, (uint32_t) i, (uint32_t) (j >> 1), 0,
                            bbo_stream(BBO_STREAM_INIT, (uint32_t) sub), w);
                    const double u = (j & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                    p.x[j] = u * (upper[j] - lower[j]) + lower[j];
                }
            }
            p.f = evaluate(p.x.data());
            swarm.push_back(p);
            fev++;
        }
        /* SHADE sorts at the end of init (shade.cpp:93); JADE sorts at the start of every
         * iterate (jade.cpp:101).  The sync form keeps the swarm sorted at generation start. */
        if (variant == 0 || sync) sort_swarm();
    }

    void sort_swarm()
    {
        if (sync) std::stable_sort(swarm.begin(), swarm.end(), point_less);
        else std::sort(swarm.begin(), swarm.end(), point_less);
    }

    /* shade.cpp:277-294 / jade.cpp:247-264 (async: draws from the global engine) */
    double mutate_async(const double *x, const double *best, const double *xr1,
            const double *xr2, double *out, double F, double CR)
    {
        const int irand = mt_int(0, n - 1);
        double cr1 = 0.;
        for (int i = 0; i < n; i++) {
            if (i == irand || mt_uniform(0., 1.) < CR) {
                out[i] = x[i] + F * (best[i] - x[i]) + F * (xr1[i] - xr2[i]);
                cr1 += 1.;
            } else {
                out[i] = x[i];
            }
        }
        return repaircr ? cr1 / n : CR;
    }

    double cauchy_async() { return std::tan(M_PI * (mt_uniform(0., 1.) - 0.5)); }

    void repair(const double *parent)
    {
        for (int j = 0; j < n; j++) {
            if (work[j] < lower[j]) {
                work[j] = (lower[j] + parent[j]) / 2.;
                repairs_lo++;
            } else if (work[j] > upper[j]) {
                work[j] = (upper[j] + parent[j]) / 2.;
                repairs_up++;
            }
        }
    }

    /* ---- the reference's generation ------------------------------------------- */
    void iterate_async()
    {
        if (variant == 1) std::sort(swarm.begin(), swarm.end(), point_less);
        int nsucc = 0;
        if (variant == 0) {
            SCR.clear();
            SF.clear();
            W.clear();
        } else {
            SCR.assign(np, 0.);
            SF.assign(np, 0.);
        }
        for (int i = 0; i < np; i++) {
            double CR, F;
            int nelite;
            if (variant == 0) {
                const int ri = mt_int(0, h - 1);
                CR = std::max(0., std::min(Z.draw() * 0.1 + MCR[ri], 1.));
                F = std::min(1., cauchy_async() * 0.1 + MF[ri]);
                while (F <= 0) F = std::min(1., cauchy_async() * 0.1 + MF[ri]);
                const double pi = mt_uniform(std::min(2. / n, 0.2), 0.2);
                nelite = std::max(1, (int) (pi * np));
            } else {
                CR = Z.draw() * 0.1 + mucr;
                CR = std::max(0., std::min(CR, 1.));
                F = -1.;
                while (F < 0.) {
                    F = cauchy_async() * 0.1 + muf;
                    F = std::min(F, 1.);
                }
                nelite = std::max(1, (int) (pelite * np));
            }
            const int ibest = mt_int(0, nelite - 1);
            int r1 = i;
            while (r1 == i) r1 = mt_int(0, np - 1);
            int r2 = i;
            const int larch = (int) arch.size();
            while (r2 == i || r2 == r1) r2 = mt_int(0, np + larch - 1);
            const double *x2 = r2 >= np ? arch[r2 - np].data() : swarm[r2].x.data();
            const double cr1 = mutate_async(swarm[i].x.data(), swarm[ibest].x.data(),
                    swarm[r1].x.data(), x2, work.data(), F, CR);
            repair(swarm[i].x.data());
            const double fwork = evaluate(work.data());
            fev++;
            if (fwork <= swarm[i].f) {
                const bool strict = fwork < swarm[i].f;
                if (archive && (variant == 1 || strict)) {
                    if (larch >= np) {
                        const int ir = mt_int(0, np - 1);
                        arch[ir] = swarm[i].x;
                    } else {
                        arch.push_back(swarm[i].x);
                    }
                }
                if (variant == 0) {
                    if (strict) {
                        SCR.push_back(cr1);
                        SF.push_back(F);
                        W.push_back(swarm[i].f - fwork);
                    }
                    swarm[i].f = fwork;
                    swarm[i].x = work;
                } else {
                    swarm[i].f = fwork;
                    swarm[i].x = work;
                    SCR[nsucc] = cr1;
                    SF[nsucc] = F;
                    nsucc++;
                }
            }
        }
        if (variant == 0) finish_shade(false);
        else finish_jade(nsucc);
        gen++;
    }

    /* shade.cpp:186-235 */
    void finish_shade(bool sync_trim)
    {
        const int lenS = (int) SCR.size();
        if (lenS > 0) {
            double crn = 0., crd = 0., fn = 0., fd = 0.;
            for (int i = 0; i < lenS; i++) {
                crn += W[i] * SCR[i];
                crd += W[i];
                fn += W[i] * SF[i] * SF[i];
                fd += W[i] * SF[i];
            }
            MCR[k - 1] = crn / crd;
            MF[k - 1] = fn / fd;
            k++;
            if (k > h) k = 1;
        }
        sort_swarm();
        const int npnew = (int) std::round((npmin - npinit) * ((1. * fev) / mfev) + npinit);
        if (npnew < np) {
            for (int i = 0; i < np - npnew; i++) swarm.pop_back();
            np = npnew;
        }
        if (archive) {
            int larch = (int) arch.size();
            int t = 0;
            while (larch > npnew) {
                if (!sync_trim) {
                    const int ir = mt_int(0, larch - 1);
                    arch.erase(arch.begin() + ir);
                } else {
                    /* sync: swap-with-last removal, slot from the ARCH stream */
                    uint32_t w[4];
                    bbo_philox(seed, (uint32_t) t, 1, (uint32_t) gen,
                            bbo_stream(BBO_STREAM_DE_ARCH, (uint32_t) sub), w);
                    const int ir = bbo_uint_below(w[0], larch);
                    arch[ir] = arch[larch - 1];
                    arch.pop_back();
                    t++;
                }
                --larch;
            }
        }
    }

    /* jade.cpp:180-205, :266-290 */
    static double mean_pow(const double *v, int cnt, int p)
    {
        double mean = 0.;
        for (int i = 0; i < cnt; i++) {
            if (p == 1) mean += (v[i] - mean) / (i + 1.);
            else mean += (v[i] * v[i] - mean) / (i + 1.);
        }
        return mean;
    }
    static double stdev(const double *v, int cnt)
    {
        double mean = 0., m2 = 0.;
        for (int i = 0; i < cnt; i++) {
            const double delta = v[i] - mean;
            mean += delta / (i + 1.);
            m2 += delta * (v[i] - mean);
        }
        return std::sqrt(m2 / cnt);
    }
    void finish_jade(int nsucc)
    {
        double meancr = 0.;
        if (nsucc > 0) {
            if (stdev(SCR.data(), nsucc) > jsigma) meancr = std::sqrt(mean_pow(SCR.data(), nsucc, 2));
            else meancr = mean_pow(SCR.data(), nsucc, 1);
        }
        mucr = (1. - cdamp) * mucr + cdamp * meancr;
        double meanf = 0.;
        if (nsucc > 0) meanf = mean_pow(SF.data(), nsucc, 2) / mean_pow(SF.data(), nsucc, 1);
        muf = (1. - cdamp) * muf + cdamp * meanf;
    }

    /* ---- the generation-synchronous form the kernels implement -------------------- */
    void philox(uint32_t c0, uint32_t c1, int stream, uint32_t w[4]) const
    {
        bbo_philox(seed, c0, c1, (uint32_t) gen, bbo_stream(stream, (uint32_t) sub), w);
    }

    void iterate_sync()
    {
        /* swarm is sorted (stable) at this point */
        const int larch0 = (int) arch.size();
        std::vector<Point> next = swarm;
        std::vector<int> ok(np, 0), strict(np, 0);
        std::vector<double> cr1v(np, 0.), Fv(np, 0.), dfv(np, 0.);
        for (int i = 0; i < np; i++) {
            uint32_t w[4];
            double z0, z1;
            bbo_normal_pair(seed, (uint32_t) i, 0, (uint32_t) gen,
                    bbo_stream(BBO_STREAM_DE_PARAM, (uint32_t) sub), &z0, &z1);
            philox((uint32_t) i, 1, BBO_STREAM_DE_PARAM, w);
            const int ri = bbo_uint_below(w[0], h);
            const int jrand = bbo_uint_below(w[1], n);
            const double up = bbo_u01(w[2], w[3]);
            const double mcr = variant == 0 ? MCR[ri] : mucr;
            const double mf = variant == 0 ? MF[ri] : muf;
            const double CR = std::max(0., std::min(z0 * 0.1 + mcr, 1.));
            double F = mf;
            bool got = false;
            for (int t = 0; t < SYNC_MAX_TRIES && !got; t++) {
                philox((uint32_t) i, (uint32_t) (16 + t), BBO_STREAM_DE_PARAM, w);
                const double u = bbo_u01(w[0], w[1]);
                F = std::min(1., std::tan(M_PI * (u - 0.5)) * 0.1 + mf);
                got = variant == 0 ? (F > 0.) : !(F < 0.);
            }
            if (!got) F = std::max(1e-8, std::min(1., mf));
            int nelite;
            if (variant == 0) {
                const double plo = std::min(2. / n, 0.2);
                const double pi = up * (0.2 - plo) + plo;
                nelite = std::max(1, (int) (pi * np));
            } else {
                nelite = std::max(1, (int) (pelite * np));
            }
            philox((uint32_t) i, 2, BBO_STREAM_DE_PARAM, w);
            const int ibest = bbo_uint_below(w[0], nelite);
            int r1 = (i + 1) % np;
            for (int t = 0; t < SYNC_MAX_TRIES; t++) {
                philox((uint32_t) i, (uint32_t) (96 + t), BBO_STREAM_DE_PARAM, w);
                const int c = bbo_uint_below(w[0], np);
                if (c != i) {
                    r1 = c;
                    break;
                }
            }
            int r2 = -1;
            for (int t = 0; t < SYNC_MAX_TRIES; t++) {
                philox((uint32_t) i, (uint32_t) (160 + t), BBO_STREAM_DE_PARAM, w);
                const int c = bbo_uint_below(w[0], np + larch0);
                if (c != i && c != r1) {
                    r2 = c;
                    break;
                }
            }
            if (r2 < 0) {
                r2 = 0;
                while (r2 == i || r2 == r1) r2++;
            }
            const double *x = swarm[i].x.data(), *best = swarm[ibest].x.data();
            const double *xr1 = swarm[r1].x.data();
            const double *xr2 = r2 >= np ? arch[r2 - np].data() : swarm[r2].x.data();
            double cnt = 0.;
            for (int j = 0; j < n; j++) {
                philox((uint32_t) i, (uint32_t) (j >> 1), BBO_STREAM_DE_CROSS, w);
                const double u = (j & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                if (j == jrand || u < CR) {
                    work[j] = x[j] + F * (best[j] - x[j]) + F * (xr1[j] - xr2[j]);
                    cnt += 1.;
                } else {
                    work[j] = x[j];
                }
            }
            repair(x);
            const double fwork = evaluate(work.data());
            cr1v[i] = repaircr ? cnt / n : CR;
            Fv[i] = F;
            if (fwork <= swarm[i].f) {
                ok[i] = 1;
                strict[i] = fwork < swarm[i].f ? 1 : 0;
                dfv[i] = swarm[i].f - fwork;
                next[i].x = work;
                next[i].f = fwork;
            }
        }
        fev += np;
        /* archive: successes in index order, push while there is room, else overwrite a
         * slot drawn from the ARCH stream (later index wins) */
        if (archive) {
            for (int i = 0; i < np; i++) {
                const bool rec = variant == 0 ? strict[i] : ok[i];
                if (!rec) continue;
                if ((int) arch.size() >= np) {
                    uint32_t w[4];
                    philox((uint32_t) i, 0, BBO_STREAM_DE_ARCH, w);
                    arch[bbo_uint_below(w[0], np)] = swarm[i].x;
                } else {
                    arch.push_back(swarm[i].x);
                }
            }
        }
        int nsucc = 0;
        if (variant == 0) {
            SCR.clear();
            SF.clear();
            W.clear();
            for (int i = 0; i < np; i++)
                if (strict[i]) {
                    SCR.push_back(cr1v[i]);
                    SF.push_back(Fv[i]);
                    W.push_back(dfv[i]);
                }
        } else {
            SCR.assign(np, 0.);
            SF.assign(np, 0.);
            for (int i = 0; i < np; i++)
                if (ok[i]) {
                    SCR[nsucc] = cr1v[i];
                    SF[nsucc] = Fv[i];
                    nsucc++;
                }
        }
        swarm.swap(next);
        if (variant == 0) {
            finish_shade(true);
        } else {
            finish_jade(nsucc);
            sort_swarm();
        }
        gen++;
    }

    void iterate()
    {
        if (sync) iterate_sync();
        else iterate_async();
    }

    bool converged()
    {
        auto getx = [](const Point &p) { return p.x.data(); };
        if (sync) return radius_converged_sync(swarm.begin(), swarm.end(), getx, n, np, tol);
        return radius_converged(swarm.begin(), swarm.end(), getx, n, np, tol);
    }

    bool optimize(int obj_, int n_, const double *lo, const double *up)
    {
        init(obj_, n_, lo, up);
        bool conv = false;
        while (fev < mfev) {
            iterate();
            if (converged()) {
                conv = true;
                break;
            }
        }
        if (!sync) std::sort(swarm.begin(), swarm.end(), point_less);
        return conv;
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) { if (cap > 0) out[0] = v; return 1; };
        auto put = [&](const std::vector<double> &v) {
            for (size_t i = 0; i < v.size() && (int) i < cap; i++) out[i] = v[i];
            return (int) v.size();
        };
        if (key == "x" || key == "f") {
            int m = 0;
            for (const auto &p : swarm) {
                if (key == "f") {
                    if (m < cap) out[m] = p.f;
                    m++;
                } else
                    for (double v : p.x) {
                        if (m < cap) out[m] = v;
                        m++;
                    }
            }
            return m;
        }
        if (key == "arch") {
            int m = 0;
            for (const auto &row : arch)
                for (double v : row) {
                    if (m < cap) out[m] = v;
                    m++;
                }
            return m;
        }
        if (key == "MCR") return put(MCR);
        if (key == "MF") return put(MF);
        if (key == "SCR") return put(SCR);
        if (key == "SF") return put(SF);
        if (key == "w") return put(W);
        if (key == "k") return put1(k);
        if (key == "np") return put1(np);
        if (key == "fev") return put1(fev);
        if (key == "larch") return put1((double) arch.size());
        if (key == "repairs_lo") return put1((double) repairs_lo);
        if (key == "repairs_up") return put1((double) repairs_up);
        if (key == "mucr") return put1(mucr);
        if (key == "muf") return put1(muf);
        return -1;
    }
};

/* ======================================================================== */
/* SaNSDE (sansde.cpp:46-300): self-adaptive DE with neighbourhood search     */
/* ======================================================================== */
struct SPoint {
    std::vector<double> x;
    double f, cr;
};
bool spoint_less(const SPoint &a, const SPoint &b) { return a.f < b.f; }

struct Sansde {
    /* parameters (sansde.cpp:46-56) */
    int mfev = 0, np = 0, ncrref = 5, npup = 50, ncrup = 25;
    double tol = 0.;
    bool repaircr = true;
    /* problem */
    int obj = 0, n = 0;
    std::vector<double> lower, upper, aux, work;
    /* state */
    int fev = 0, it = 0;
    long repairs_lo = 0, repairs_up = 0;   /* coordinates repair() moved, per side (read-only) */
    double p = 0.5, fp = 0.5, crrec = 0., crdeltaf = 0., crm = 0.5;
    int pns[2] = { 0, 0 }, pnf[2] = { 0, 0 };
    double fpns[2] = { 0., 0. }, fpnf[2] = { 0., 0. };
    std::vector<SPoint> swarm;
    /* mode */
    bool sync = false;
    int rng_mode = RNG_MT;
    uint64_t seed = 0;
    int sub = 0;
    NormalCache Z;

    double evaluate(const double *q) { return bbo_objective_eval(obj, n, q, aux.data()); }

    void philox(uint32_t c0, uint32_t c1, int stream, uint32_t w[4]) const
    {
        bbo_philox(seed, c0, c1, (uint32_t) it, bbo_stream(stream, (uint32_t) sub), w);
    }

    /* sansde.cpp:58-94 */
    void init(int obj_, int n_, const double *lo, const double *up)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        fev = it = 0;
        repairs_lo = repairs_up = 0;
        p = fp = 0.5;
        crrec = crdeltaf = 0.;
        crm = 0.5;
        pns[0] = pns[1] = pnf[0] = pnf[1] = 0;
        fpns[0] = fpns[1] = fpnf[0] = fpnf[1] = 0.;
        work.assign(n, 0.);
        swarm.clear();
        for (int i = 0; i < np; i++) {
            SPoint q;
            q.x.resize(n);
            for (int j = 0; j < n; j++) {
                if (rng_mode == RNG_MT) {
                    q.x[j] = mt_uniform(lower[j], upper[j]);
                } else {
                    uint32_t w[4];
                    bbo_philox(seed, (uint32_t) i, (uint32_t) (j >> 1), 0,
                            bbo_stream(BBO_STREAM_INIT, (uint32_t) sub), w);
                    const double u = (j & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                    q.x[j] = u * (upper[j] - lower[j]) + lower[j];
                }
            }
            q.f = evaluate(q.x.data());
            q.cr = 0.5;
            swarm.push_back(q);
            fev++;
        }
    }

    void repair(const double *parent)
    {
        for (int j = 0; j < n; j++) {
            if (work[j] < lower[j]) {
                work[j] = (lower[j] + parent[j]) / 2.;
                repairs_lo++;
            } else if (work[j] > upper[j]) {
                work[j] = (upper[j] + parent[j]) / 2.;
                repairs_up++;
            }
        }
    }

    void mutate_into_work(const double *x, const double *best, const double *xr1,
            const double *xr2, const double *xr3, double F, int strat)
    {
        if (strat == 0)
            for (int j = 0; j < n; j++) work[j] = xr1[j] + F * (xr2[j] - xr3[j]);
        else
            for (int j = 0; j < n; j++)
                work[j] = x[j] + F * (best[j] - x[j]) + F * (xr1[j] - xr2[j]);
    }

    /* sansde.cpp:213-234: strategy, crossover and their adaptation counters */
    void adapt()
    {
        it++;
        if (it > 0 && it % npup == 0) {
            const int pnsf0 = pns[0] + pnf[0];
            const int pnsf1 = pns[1] + pnf[1];
            p = (1. * pns[0] * pnsf1) / (pns[1] * pnsf0 + pns[0] * pnsf1);
            pns[0] = pns[1] = pnf[0] = pnf[1] = 0;
        }
        if (it > 0 && it % ncrup == 0) {
            if (crdeltaf > 0) crm = crrec / crdeltaf;
            crrec = crdeltaf = 0.;
        }
        if (it > 0 && it % ncrup == 0) {
            const double fpnsf0 = fpns[0] + fpnf[0];
            const double fpnsf1 = fpns[1] + fpnf[1];
            fp = (1. * fpns[0] * fpnsf1) / (fpns[1] * fpnsf0 + fpns[0] * fpnsf1);
            fpns[0] = fpns[1] = fpnf[0] = fpnf[1] = 0.;
        }
    }

    /* ---- the reference's generation (sansde.cpp:96-234): in-place, global mt19937 ---- */
    void iterate_async()
    {
        std::sort(swarm.begin(), swarm.end(), spoint_less);
        for (int i = 0; i < np; i++) {
            if (it % ncrref == 0) {
                swarm[i].cr = Z.draw() * 0.1 + crm;
                swarm[i].cr = std::max(0., std::min(swarm[i].cr, 1.));
            }
            const int ifstrat = mt_uniform(0., 1.) < fp ? 0 : 1;
            double F = -1.;
            while (F < 0.) {
                if (ifstrat == 0) F = Z.draw() * 0.3 + 0.5;
                else F = std::tan(M_PI * (mt_uniform(0., 1.) - 0.5));
                F = std::min(F, 1.);
            }
            int r1 = i;
            while (r1 == i) r1 = mt_int(0, np - 1);
            int r2 = i;
            while (r2 == i || r2 == r1) r2 = mt_int(0, np - 1);
            int r3 = i;
            while (r3 == i || r3 == r1 || r3 == r2) r3 = mt_int(0, np - 1);
            const int istrat = mt_uniform(0., 1.) < p ? 0 : 1;
            mutate_into_work(swarm[i].x.data(), swarm[0].x.data(), swarm[r1].x.data(),
                    swarm[r2].x.data(), swarm[r3].x.data(), F, istrat);
            /* crossover (sansde.cpp:281-295): the uniform is drawn for every coordinate */
            const int irand = mt_int(0, n - 1);
            double cr1 = 0.;
            for (int j = 0; j < n; j++) {
                if (mt_uniform(0., 1.) <= swarm[i].cr || j == irand) cr1 += 1.;
                else work[j] = swarm[i].x[j];
            }
            cr1 = repaircr ? cr1 / n : swarm[i].cr;
            repair(swarm[i].x.data());
            const double fwork = evaluate(work.data());
            fev++;
            if (fwork < swarm[i].f) {
                pns[istrat]++;
                const double deltaf = swarm[i].f - fwork;
                crrec += cr1 * deltaf;
                crdeltaf += deltaf;
                fpns[ifstrat] += F;
                swarm[i].f = fwork;
                swarm[i].x = work;
            } else {
                pnf[istrat]++;
                fpnf[ifstrat] += F;
            }
        }
        adapt();
    }

    /* ---- generation-synchronous form (what the device computes): every trial is built from
     * the population of the generation start, draws are Philox words keyed by (individual,
     * purpose, generation) -- bboptpy_amd/csrc/bbo_de_kernels.hpp: sansde_generation ---- */
    void iterate_sync()
    {
        std::stable_sort(swarm.begin(), swarm.end(), spoint_less);
        std::vector<SPoint> next = swarm;
        std::vector<int> okv(np, 0), isv(np, 0), ifv(np, 0);
        std::vector<double> cr1v(np, 0.), Fv(np, 0.), dfv(np, 0.);
        for (int i = 0; i < np; i++) {
            uint32_t w[4];
            double cr = swarm[i].cr;
            if (it % ncrref == 0) {
                double z0, z1;
                bbo_normal_pair(seed, (uint32_t) i, 0, (uint32_t) it,
                        bbo_stream(BBO_STREAM_DE_PARAM, (uint32_t) sub), &z0, &z1);
                cr = std::max(0., std::min(z0 * 0.1 + crm, 1.));
            }
            philox((uint32_t) i, 1, BBO_STREAM_DE_PARAM, w);
            const int ifstrat = bbo_u01(w[0], w[1]) < fp ? 0 : 1;
            const int istrat = bbo_u01(w[2], w[3]) < p ? 0 : 1;
            double F = 0.5;
            bool got = false;
            for (int t = 0; t < SYNC_MAX_TRIES && !got; t++) {
                if (ifstrat == 0) {
                    double z0, z1;
                    bbo_normal_pair(seed, (uint32_t) i, (uint32_t) (16 + t), (uint32_t) it,
                            bbo_stream(BBO_STREAM_DE_PARAM, (uint32_t) sub), &z0, &z1);
                    F = z0 * 0.3 + 0.5;
                } else {
                    philox((uint32_t) i, (uint32_t) (16 + t), BBO_STREAM_DE_PARAM, w);
                    F = std::tan(M_PI * (bbo_u01(w[0], w[1]) - 0.5));
                }
                F = std::min(F, 1.);
                got = !(F < 0.);
            }
            if (!got) F = 0.5;
            int r[3] = { -1, -1, -1 };
            for (int q = 0; q < 3; q++) {
                for (int t = 0; t < SYNC_MAX_TRIES && r[q] < 0; t++) {
                    philox((uint32_t) i, (uint32_t) (96 + 64 * q + t), BBO_STREAM_DE_PARAM, w);
                    const int c = bbo_uint_below(w[0], np);
                    if (c != i && c != r[0] && c != r[1]) r[q] = c;
                }
                for (int c = 0; r[q] < 0; c++)
                    if (c != i && c != r[0] && c != r[1]) r[q] = c;
            }
            philox((uint32_t) i, 2, BBO_STREAM_DE_PARAM, w);
            const int jrand = bbo_uint_below(w[0], n);
            const double *x = swarm[i].x.data();
            mutate_into_work(x, swarm[0].x.data(), swarm[r[0]].x.data(), swarm[r[1]].x.data(),
                    swarm[r[2]].x.data(), F, istrat);
            double cnt = 0.;
            for (int j = 0; j < n; j++) {
                philox((uint32_t) i, (uint32_t) (j >> 1), BBO_STREAM_DE_CROSS, w);
                const double u = (j & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                if (u <= cr || j == jrand) cnt += 1.;
                else work[j] = x[j];
            }
            repair(x);
            const double fwork = evaluate(work.data());
            cr1v[i] = repaircr ? cnt / n : cr;
            Fv[i] = F;
            isv[i] = istrat;
            ifv[i] = ifstrat;
            next[i].cr = cr;
            if (fwork < swarm[i].f) {
                okv[i] = 1;
                dfv[i] = swarm[i].f - fwork;
                next[i].x = work;
                next[i].f = fwork;
            }
        }
        fev += np;
        for (int i = 0; i < np; i++) {
            if (okv[i]) {
                pns[isv[i]]++;
                crrec += cr1v[i] * dfv[i];
                crdeltaf += dfv[i];
                fpns[ifv[i]] += Fv[i];
            } else {
                pnf[isv[i]]++;
                fpnf[ifv[i]] += Fv[i];
            }
        }
        swarm.swap(next);
        adapt();
    }

    void iterate()
    {
        if (sync) iterate_sync();
        else iterate_async();
    }

    bool converged()
    {
        auto getx = [](const SPoint &q) { return q.x.data(); };
        if (sync) return radius_converged_sync(swarm.begin(), swarm.end(), getx, n, np, tol);
        return radius_converged(swarm.begin(), swarm.end(), getx, n, np, tol);
    }

    void sort_swarm()
    {
        if (sync) std::stable_sort(swarm.begin(), swarm.end(), spoint_less);
        else std::sort(swarm.begin(), swarm.end(), spoint_less);
    }

    /* sansde.cpp:241-254 */
    bool optimize(int obj_, int n_, const double *lo, const double *up)
    {
        init(obj_, n_, lo, up);
        bool conv = false;
        while (fev < mfev) {
            iterate();
            if (converged()) {
                conv = true;
                break;
            }
        }
        sort_swarm();
        return conv;
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) {
            if (cap >= 1) out[0] = v;
            return 1;
        };
        if (key == "x" || key == "f" || key == "cr") {
            int m = 0;
            for (const auto &q : swarm) {
                if (key == "x") {
                    for (double v : q.x) {
                        if (m < cap) out[m] = v;
                        m++;
                    }
                } else {
                    if (m < cap) out[m] = key == "f" ? q.f : q.cr;
                    m++;
                }
            }
            return m;
        }
        if (key == "np") return put1(np);
        if (key == "fev") return put1(fev);
        if (key == "it") return put1(it);
        if (key == "p") return put1(p);
        if (key == "fp") return put1(fp);
        if (key == "crm") return put1(crm);
        if (key == "crrec") return put1(crrec);
        if (key == "crdeltaf") return put1(crdeltaf);
        if (key == "repairs_lo") return put1((double) repairs_lo);
        if (key == "repairs_up") return put1((double) repairs_up);
        if (key == "pns" || key == "pnf") {
            const int *a = key == "pns" ? pns : pnf;
            if (cap >= 2) { out[0] = a[0]; out[1] = a[1]; }
            return 2;
        }
        if (key == "fpns" || key == "fpnf") {
            const double *a = key == "fpns" ? fpns : fpnf;
            if (cap >= 2) { out[0] = a[0]; out[1] = a[1]; }
            return 2;
        }
        return -1;
    }
};

/* ======================================================================== */
/* CSO, competitive swarm optimizer (cso.cpp:46-276)                          */
/* ======================================================================== */
struct CsoParticle {
    std::vector<double> x, v, mean;
    double f;
    /* cso.cpp:101-108 stores POINTERS to the neighbouring SLOTS of the slot the particle was
     * born in; the structs are later shuffled and sorted (moved between slots) but keep those
     * pointers, so a particle's ring neighbours are whoever currently sits next to its birth
     * slot.  `home` is that birth slot. */
    int home;
};
bool cso_less(const CsoParticle &a, const CsoParticle &b) { return a.f < b.f; }

struct Cso {
    /* parameters (cso.cpp:46-65) */
    int mfev = 0, np = 0, pcompete = 3;
    double stol = 0., vmax = 0.2;
    bool ring = false, correct = true;
    /* problem */
    int obj = 0, n = 0;
    std::vector<double> lower, upper, aux;
    /* state */
    int fev = 0, ngroup = 0, gen = 0, ibest = 0;
    std::vector<double> mean, meanw, phil, phih;
    std::vector<CsoParticle> swarm;
    /* mode */
    bool sync = false;
    int rng_mode = RNG_MT;
    uint64_t seed = 0;
    int sub = 0;

    double evaluate(const double *q) { return bbo_objective_eval(obj, n, q, aux.data()); }

    void philox(uint32_t c0, uint32_t c1, int stream, uint32_t w[4]) const
    {
        bbo_philox(seed, c0, c1, (uint32_t) gen, bbo_stream(stream, (uint32_t) sub), w);
    }

    void configure()   /* the constructor's adjustments, cso.cpp:53-64 */
    {
        if (pcompete < 2) pcompete = 2;
        while (np % pcompete != 0) np++;
    }

    /* cso.cpp:196-217 */
    void compute_phi(int m)
    {
        phil.assign(pcompete, 0.);
        phih.assign(pcompete, 0.);
        if (pcompete == 2) {
            if (m <= 100) {
                phil[0] = phih[0] = 0.;
            } else {
                phil[0] = std::max(0., 0.14 * std::log(m) - 0.3);
                phih[0] = std::max(0., 0.27 * std::log(m) - 0.51);
            }
            std::fill(phil.begin(), phil.end(), phil[0]);
            std::fill(phih.begin(), phih.end(), phih[0]);
        } else {
            std::fill(phil.begin(), phil.end(), 0.);
            std::fill(phih.begin(), phih.end(), 0.3);
        }
    }

    /* cso.cpp:67-112 */
    void init(int obj_, int n_, const double *lo, const double *up)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        configure();
        compute_phi(np);
        gen = 0;
        swarm.clear();
        for (int i = 0; i < np; i++) {
            CsoParticle q;
            q.x.resize(n);
            q.v.assign(n, 0.);
            q.mean.assign(n, 0.);
            for (int j = 0; j < n; j++) {
                if (rng_mode == RNG_MT) {
                    q.x[j] = mt_uniform(lower[j], upper[j]);
                } else {
                    uint32_t w[4];
                    bbo_philox(seed, (uint32_t) i, (uint32_t) (j >> 1), 0,
                            bbo_stream(BBO_STREAM_INIT, (uint32_t) sub), w);
                    const double u = (j & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                    q.x[j] = u * (upper[j] - lower[j]) + lower[j];
                }
            }
            q.f = evaluate(q.x.data());
            q.home = i;
            swarm.push_back(q);
        }
        ngroup = np / pcompete;
        fev = np;
        ibest = 0;
        mean.assign(n, 0.);
        meanw.assign(n, 0.);
    }

    /* libstdc++-11 std::shuffle over the global mt19937 (bits/stl_algo.h:3730-3790): two swap
     * positions per draw while (range)^2 fits the generator's range */
    void std_shuffle()
    {
        const uint64_t urng_range = 0xffffffffull;
        const uint64_t urange = (uint64_t) np;
        if (np < 2) return;
        if (urng_range / urange >= urange) {
            size_t i = 1;
            if ((urange % 2) == 0) {
                std::swap(swarm[i], swarm[(size_t) mt_int(0, 1)]);
                i++;
            }
            while (i != (size_t) np) {
                const uint64_t swap_range = (uint64_t) i + 1;
                const uint64_t b1 = swap_range + 1;
                const uint64_t xx = (uint64_t) (uint32_t) mt_int(0, (int) (swap_range * b1 - 1));
                std::swap(swarm[i], swarm[(size_t) (xx / b1)]);
                i++;
                std::swap(swarm[i], swarm[(size_t) (xx % b1)]);
                i++;
            }
            return;
        }
        for (size_t i = 1; i < (size_t) np; i++)
            std::swap(swarm[i], swarm[(size_t) mt_int(0, (int) i)]);
    }

    /* the sync shuffle: a keyed bijection of the slots, new slot s takes the occupant of slot
     * perm(s).  perm = 4-round Feistel network on 2 kb bits (kb = half the bits of np - 1,
     * rounded up), round function = one Philox word keyed by (half-word, round, generation),
     * cycle-walked back into [0, np).  No sort, O(1) per slot -- what the device computes
     * (bbo_cso_kernels.hpp: cso_perm). */
    uint32_t feistel_perm(uint32_t s0, int kb) const
    {
        const uint32_t mask = (1u << kb) - 1u;
        uint32_t x = s0;
        do {
            uint32_t L = x >> kb, R = x & mask;
            for (int r = 0; r < 4; r++) {
                uint32_t w[4];
                philox(R, (uint32_t) (8 + r), BBO_STREAM_PSO_CTRL, w);
                const uint32_t t = L ^ (w[0] & mask);
                L = R;
                R = t;
            }
            x = (L << kb) | R;
        } while (x >= (uint32_t) np);
        return x;
    }

    void philox_shuffle()
    {
        int bits = 1;
        while ((1u << bits) < (uint32_t) np) bits++;
        const int kb = (bits + 1) / 2;
        std::vector<CsoParticle> next(np);
        for (int s = 0; s < np; s++) next[s] = swarm[feistel_perm((uint32_t) s, kb)];
        swarm.swap(next);
    }

    /* cso.cpp:219-276; u(k): the k-th uniform of this loser's coordinate j */
    void compete(int istart)
    {
        for (int p = istart + pcompete - 1; p > istart; p--) {
            double phi;
            uint32_t w[4];
            if (rng_mode == RNG_MT) {
                phi = mt_uniform(phil[p - istart], phih[p - istart]);
            } else {
                philox((uint32_t) p, 1, BBO_STREAM_PSO_CTRL, w);
                phi = bbo_u01(w[0], w[1]) * (phih[p - istart] - phil[p - istart]) + phil[p - istart];
            }
            const CsoParticle &parent = swarm[p - 1];
            CsoParticle &part = swarm[p];
            for (int i = 0; i < n; i++) {
                double xmean;
                if (p == istart + 1) xmean = ring ? part.mean[i] : mean[i];
                else xmean = meanw[i];
                double r1, r2, r3;
                if (rng_mode == RNG_MT) {
                    r1 = mt_uniform(0., 1.);
                    r2 = mt_uniform(0., 1.);
                    r3 = mt_uniform(0., 1.);
                } else {
                    /* slot p, coordinate pair pj = i / 2: blocks 3 pj and 3 pj + 1 hold (r1, r2)
                     * of the even / odd coordinate, block 3 pj + 2 holds r3 of both */
                    const int pj = i >> 1;
                    philox((uint32_t) p, (uint32_t) (3 * pj + (i & 1)), BBO_STREAM_PSO_R, w);
                    r1 = bbo_u01(w[0], w[1]);
                    r2 = bbo_u01(w[2], w[3]);
                    philox((uint32_t) p, (uint32_t) (3 * pj + 2), BBO_STREAM_PSO_R, w);
                    r3 = (i & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                }
                part.v[i] = r1 * part.v[i] + r2 * (parent.x[i] - part.x[i])
                        + phi * r3 * (xmean - part.x[i]);
                const double maxv = vmax * (upper[i] - lower[i]);
                part.v[i] = std::max(-maxv, std::min(part.v[i], maxv));
                part.x[i] += part.v[i];
                if (correct) part.x[i] = std::max(lower[i], std::min(part.x[i], upper[i]));
            }
            part.f = evaluate(part.x.data());
            fev++;
        }
    }

    /* cso.cpp:114-158 */
    void iterate()
    {
        if (ring) {
            /* neighbours = current occupants of the slots next to the particle's birth slot */
            std::vector<std::vector<double>> snap(np);
            for (int s = 0; s < np; s++) snap[s] = swarm[s].x;
            for (auto &q : swarm) {
                const int il = (q.home - 1 + np) % np, ir = (q.home + 1) % np;
                /* the reference reads the LIVE slots while it walks the swarm; only x is read
                 * and x does not change in this loop, so a snapshot is the same thing */
                for (int i = 0; i < n; i++)
                    q.mean[i] = (snap[il][i] + q.x[i] + snap[ir][i]) / 3.;
            }
        } else {
            std::fill(mean.begin(), mean.end(), 0.);
            for (const auto &q : swarm)
                for (int i = 0; i < n; i++) mean[i] += q.x[i] / np;
        }
        std::fill(meanw.begin(), meanw.end(), 0.);
        if (rng_mode == RNG_MT) std_shuffle();
        else philox_shuffle();
        for (int p = 0; p < np; p += pcompete) {
            if (sync) std::stable_sort(swarm.begin() + p, swarm.begin() + p + pcompete, cso_less);
            else std::sort(swarm.begin() + p, swarm.begin() + p + pcompete, cso_less);
            for (int i = 0; i < n; i++) meanw[i] += swarm[p].x[i] / ngroup;
        }
        for (int i = 0; i < np; i += pcompete) compete(i);
        ibest = 0;
        for (int s = 0; s < np; s++)
            if (swarm[s].f < swarm[ibest].f) ibest = s;
        gen++;
    }

    bool converged()
    {
        auto getx = [](const CsoParticle &q) { return q.x.data(); };
        if (sync) return radius_converged_sync(swarm.begin(), swarm.end(), getx, n, np, stol);
        return radius_converged(swarm.begin(), swarm.end(), getx, n, np, stol);
    }

    bool optimize(int obj_, int n_, const double *lo, const double *up)
    {
        init(obj_, n_, lo, up);
        bool conv = false;
        while (fev < mfev) {
            iterate();
            if (converged()) {
                conv = true;
                break;
            }
        }
        return conv;
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) {
            if (cap >= 1) out[0] = v;
            return 1;
        };
        if (key == "x" || key == "v" || key == "pmean" || key == "f" || key == "home") {
            int m = 0;
            for (const auto &q : swarm) {
                if (key == "f" || key == "home") {
                    if (m < cap) out[m] = key == "f" ? q.f : (double) q.home;
                    m++;
                } else {
                    const auto &src = key == "x" ? q.x : key == "v" ? q.v : q.mean;
                    for (double v : src) {
                        if (m < cap) out[m] = v;
                        m++;
                    }
                }
            }
            return m;
        }
        if (key == "mean" || key == "meanw" || key == "phil" || key == "phih") {
            const auto &src = key == "mean" ? mean : key == "meanw" ? meanw : key == "phil" ? phil
                                                                                            : phih;
            for (size_t i = 0; i < src.size() && (int) i < cap; i++) out[i] = src[i];
            return (int) src.size();
        }
        if (key == "xbest") {
            for (int i = 0; i < n && i < cap; i++) out[i] = swarm[ibest].x[i];
            return n;
        }
        if (key == "fbest") return put1(swarm[ibest].f);
        if (key == "np") return put1(np);
        if (key == "fev") return put1(fev);
        if (key == "it") return put1(gen);
        return -1;
    }
};

/* ======================================================================== */
/* CCPSO2, cooperatively coevolving PSO (ccpso.cpp:51-454; Li & Yao 2012)     */
/* ======================================================================== */
struct Ccpso {
    /* parameters (ccpso.cpp:51-64).  `local` (null = the binding's default) is the optimizer
     * localSearch() runs on the per-swarm weights every `localfreq` generations; this
     * restatement takes a CMA-ES variant for it (owned). */
    Cma *local = nullptr;
    int localfreq = 10;
    int nlocal = 0;                 /* local searches so far */
    uint64_t local_seed0 = 0;       /* Philox mode: search q draws with seed local_seed0 + q */
    /* The reference's Cmaes::init resize()s _b and _c without clearing (cmaes.cpp:53-54): a
     * second search starts from the first one's matrices (diagonals reset to 1), and a search
     * in MORE dimensions than the one before indexes past the old rows -- undefined behaviour
     * (heap corruption observed here), so parity with the reference is only defined while the
     * number of swarms does not grow (a single `pps` entry).  local_fresh = true instead starts
     * every search from B = C = I: what the device does (documented deviation). */
    bool local_fresh = false;
    std::vector<double> wlb, wub, wguess;
    ~Ccpso() { delete local; }
    int mfev = 0, np = 0;
    double stol = 0., phat0 = -1.;
    bool correct = true, adaptp = true;
    std::vector<int> pps;
    /* problem */
    int obj = 0, n = 0;
    std::vector<double> lower, upper, aux;
    /* state */
    int fev = 0, gen = 0, nswarm = 0, cpswarm = 0, is = -1;
    bool improved = false;
    double fyhat = 0., phat = 0.5;
    std::vector<double> X, Y, yhat, temp, fX, fY;      /* X, Y: np x n; fX, fY: nswarm x np */
    std::vector<int> kidx, ibest, strat, range;        /* kidx: nswarm x cpswarm */
    /* mode */
    bool sync = false;
    int rng_mode = RNG_MT;
    uint64_t seed = 0;
    int sub = 0;
    NormalCache Z;

    double evaluate_vec(const double *q) { return bbo_objective_eval(obj, n, q, aux.data()); }

    void philox(uint32_t c0, uint32_t c1, int stream, uint32_t w[4]) const
    {
        bbo_philox(seed, c0, c1, (uint32_t) gen, bbo_stream(stream, (uint32_t) sub), w);
    }

    /* ccpso.cpp:66-112 */
    void init(int obj_, int n_, const double *lo, const double *up)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        /* (the reference tests `_phat < 1.` on an uninitialised member here; the intended
         * reading -- adapt unless a probability in (0, 1) was given -- is taken) */
        adaptp = !(phat0 > 0. && phat0 < 1.);
        fev = 0;
        X.assign((size_t) np * n, 0.);
        Y.assign((size_t) np * n, 0.);
        yhat.assign(n, 0.);
        fyhat = std::numeric_limits<double>::infinity();
        gen = 0;
        for (int ip = 0; ip < np; ip++) {
            for (int i = 0; i < n; i++) {
                double v;
                if (rng_mode == RNG_MT) {
                    v = mt_uniform(lower[i], upper[i]);
                } else {
                    uint32_t w[4];
                    bbo_philox(seed, (uint32_t) ip, (uint32_t) (i >> 1), 0,
                            bbo_stream(BBO_STREAM_INIT, (uint32_t) sub), w);
                    const double u = (i & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                    v = u * (upper[i] - lower[i]) + lower[i];
                }
                X[(size_t) ip * n + i] = Y[(size_t) ip * n + i] = v;
            }
            const double fx = evaluate_vec(&X[(size_t) ip * n]);
            if (fx < fyhat) {
                fyhat = fx;
                std::copy(X.begin() + (size_t) ip * n, X.begin() + (size_t) (ip + 1) * n,
                        yhat.begin());
            }
        }
        fev = np;
        temp.assign(n, 0.);
        range.assign(n, 0);
        improved = false;
        is = -1;
        nswarm = cpswarm = 0;
        phat = adaptp ? 0.5 : phat0;
    }

    /* libstdc++-11 std::shuffle of `range` over the global mt19937 (see Cso::std_shuffle) */
    void std_shuffle_range()
    {
        const uint64_t urng_range = 0xffffffffull, urange = (uint64_t) n;
        if (n < 2) return;
        if (urng_range / urange >= urange) {
            size_t i = 1;
            if ((urange % 2) == 0) {
                std::swap(range[i], range[(size_t) mt_int(0, 1)]);
                i++;
            }
            while (i != (size_t) n) {
                const uint64_t swap_range = (uint64_t) i + 1, b1 = swap_range + 1;
                const uint64_t xx = (uint64_t) (uint32_t) mt_int(0, (int) (swap_range * b1 - 1));
                std::swap(range[i], range[(size_t) (xx / b1)]);
                i++;
                std::swap(range[i], range[(size_t) (xx % b1)]);
                i++;
            }
            return;
        }
        for (size_t i = 1; i < (size_t) n; i++) std::swap(range[i], range[(size_t) mt_int(0, (int) i)]);
    }

    /* sync mode: the keyed Feistel bijection of Cso::feistel_perm, over the n coordinates */
    uint32_t feistel_perm(uint32_t s0, int kb) const
    {
        const uint32_t mask = (1u << kb) - 1u;
        uint32_t x = s0;
        do {
            uint32_t L = x >> kb, R = x & mask;
            for (int r = 0; r < 4; r++) {
                uint32_t w[4];
                philox(R, (uint32_t) (8 + r), BBO_STREAM_PSO_CTRL, w);
                const uint32_t t = L ^ (w[0] & mask);
                L = R;
                R = t;
            }
            x = (L << kb) | R;
        } while (x >= (uint32_t) n);
        return x;
    }

    /* ccpso.cpp:188-231 */
    void randomize_components()
    {
        const int is0 = is;
        if (!improved) {
            if (rng_mode == RNG_MT) {
                is = mt_int(0, (int) pps.size() - 1);
            } else {
                uint32_t w[4];
                philox(0, 0, BBO_STREAM_PSO_CTRL, w);
                is = bbo_uint_below(w[0], (int) pps.size());
            }
        }
        if (is != is0) {
            cpswarm = pps[is];
            if (cpswarm <= 0 || cpswarm > n || n % cpswarm != 0)
                throw std::runtime_error("Error [CC-PSO]: invalid component size.");
            nswarm = n / cpswarm;
            kidx.assign((size_t) nswarm * cpswarm, 0);
            fX.assign((size_t) nswarm * np, 0.);
            fY.assign((size_t) nswarm * np, 0.);
            ibest.assign((size_t) nswarm * np, 0);
            strat.assign((size_t) nswarm * np, 0);
        }
        if (rng_mode == RNG_MT) {
            for (int j = 0; j < n; j++) range[j] = j;
            std_shuffle_range();
        } else {
            int bits = 1;
            while ((1u << bits) < (uint32_t) n) bits++;
            const int kb = (bits + 1) / 2;
            for (int j = 0; j < n; j++) range[j] = (int) feistel_perm((uint32_t) j, kb);
        }
        for (int q = 0; q < n; q++) kidx[q] = range[q];
    }

    /* ccpso.cpp:150-168: the context vector with the components of swarm j replaced */
    double evaluate_ctx(int j, const double *src_row)
    {
        const int *kk = &kidx[(size_t) j * cpswarm];
        for (int q = 0; q < cpswarm; q++) {
            temp[kk[q]] = yhat[kk[q]];
            yhat[kk[q]] = src_row[kk[q]];
        }
        const double fit = evaluate_vec(yhat.data());
        fev++;
        for (int q = 0; q < cpswarm; q++) yhat[kk[q]] = temp[kk[q]];
        return fit;
    }

    /* ccpso.cpp:233-333 */
    void update_swarm()
    {
        eval_tables(0, nswarm);
        apply_tables();
    }

    /* the 2 np context-vector evaluations of the swarms [j0, j1), ccpso.cpp:241-247 */
    void eval_tables(int j0, int j1)
    {
        for (int j = j0; j < j1; j++)
            for (int i = 0; i < np; i++) {
                fX[(size_t) j * np + i] = evaluate_ctx(j, &X[(size_t) i * n]);
                fY[(size_t) j * np + i] = evaluate_ctx(j, &Y[(size_t) i * n]);
            }
    }

    /* ---- swarm groups sharded over ranks (the device's bbo_ccpso_* entry points restated) --- */
    int shard_rank = 0, shard_world = 1;
    int shard_lo(int r) const { return (int) ((long) nswarm * r / shard_world); }
    void phase(int which)
    {
        if (which == 0) {
            randomize_components();
            eval_tables(shard_lo(shard_rank), shard_lo(shard_rank + 1));
        } else {
            apply_tables();
            update_position();
            gen++;
        }
    }
    void export_tables(double *out) const      /* fX | fY at full capacity n * np */
    {
        const size_t cap = (size_t) n * np;
        for (size_t q = 0; q < 2 * cap; q++) out[q] = 0.;
        for (size_t q = 0; q < (size_t) nswarm * np; q++) {
            out[q] = fX[q];
            out[cap + q] = fY[q];
        }
    }
    void merge_tables(const double *gathered, int world)
    {
        const size_t cap = (size_t) n * np;
        for (int r = 0; r < world; r++)
            for (int j = shard_lo(r); j < shard_lo(r + 1); j++)
                for (int i = 0; i < np; i++) {
                    const size_t q = (size_t) j * np + i;
                    fX[q] = gathered[(size_t) r * 2 * cap + q];
                    fY[q] = gathered[(size_t) r * 2 * cap + cap + q];
                }
        /* the evaluations the other ranks made count here too (the state is replicated) */
        fev += 2 * np * (nswarm - (shard_lo(shard_rank + 1) - shard_lo(shard_rank)));
    }

    /* ccpso.cpp:251-333 on the filled tables */
    void apply_tables()
    {
        bool yhatupdate = false;
        std::vector<double> saved = yhat;
        for (int j = 0; j < nswarm; j++) {
            const int *kk = &kidx[(size_t) j * cpswarm];
            for (int i = 0; i < np; i++) {
                if (fX[(size_t) j * np + i] < fY[(size_t) j * np + i])
                    for (int q = 0; q < cpswarm; q++)
                        Y[(size_t) i * n + kk[q]] = X[(size_t) i * n + kk[q]];
                /* (fY is NOT refreshed after the copy, and _fyhat is not lowered inside this
                 * loop: the last qualifying particle of a swarm wins -- kept) */
                if (fY[(size_t) j * np + i] < fyhat) {
                    for (int q = 0; q < cpswarm; q++) yhat[kk[q]] = Y[(size_t) i * n + kk[q]];
                    yhatupdate = true;
                }
                const int idx3[3] = { (i - 1 + np) % np, i, (i + 1) % np };
                int imin = 0;
                for (int q = 1; q < 3; q++)
                    if (fY[(size_t) j * np + idx3[q]] < fY[(size_t) j * np + idx3[imin]]) imin = q;
                ibest[(size_t) j * np + i] = idx3[imin];
            }
        }
        const double fyhat0 = fyhat;
        if (yhatupdate) {
            fyhat = evaluate_vec(yhat.data());
            fev++;
        }
        improved = fyhat < fyhat0;
        if (!improved) {
            fyhat = fyhat0;
            yhat = saved;
        }
        if (gen > 0 && adaptp) {
            int cs = 0, ns = 0, ctot = 0, ntot = 0;
            for (int j = 0; j < nswarm; j++)
                for (int i = 0; i < np; i++) {
                    const size_t q = (size_t) j * np + i;
                    if (fX[q] < fY[q]) {
                        if (strat[q] == 0) cs++;
                        else ns++;
                    }
                    if (strat[q] == 0) ctot++;
                    else ntot++;
                }
            const double crate = 1. * cs / std::max(1, ctot);
            const double nrate = 1. * ns / std::max(1, ntot);
            phat = std::max(0.05, std::min(crate / std::max(1., crate + nrate), 0.95));
        }
    }

    /* ccpso.cpp:335-371 */
    void update_position()
    {
        for (int j = 0; j < nswarm; j++) {
            const int *kk = &kidx[(size_t) j * cpswarm];
            for (int i = 0; i < np; i++) {
                double us;
                uint32_t w[4];
                if (rng_mode == RNG_MT) {
                    us = mt_uniform(0., 1.);
                } else {
                    philox((uint32_t) i, (uint32_t) (16 + j), BBO_STREAM_PSO_CTRL, w);
                    us = bbo_u01(w[0], w[1]);
                }
                const bool cauchy = us < phat;
                const int ihat = ibest[(size_t) j * np + i];
                for (int q = 0; q < cpswarm; q++) {
                    const int d = kk[q];
                    double dev;
                    if (rng_mode == RNG_MT) {
                        dev = cauchy ? std::tan(M_PI * (mt_uniform(0., 1.) - 0.5)) : Z.draw();
                    } else if (cauchy) {
                        philox((uint32_t) i, (uint32_t) (d >> 1), BBO_STREAM_PSO_R, w);
                        const double u = (d & 1) ? bbo_u01(w[2], w[3]) : bbo_u01(w[0], w[1]);
                        dev = std::tan(M_PI * (u - 0.5));
                    } else {
                        double z0, z1;
                        bbo_normal_pair(seed, (uint32_t) i, (uint32_t) (d >> 1), (uint32_t) gen,
                                bbo_stream(BBO_STREAM_PSO_R, (uint32_t) sub), &z0, &z1);
                        dev = (d & 1) ? z1 : z0;
                    }
                    const double sigma = std::fabs(Y[(size_t) i * n + d] - Y[(size_t) ihat * n + d]);
                    double v = (cauchy ? Y[(size_t) i * n + d] : Y[(size_t) ihat * n + d]) + dev * sigma;
                    if (correct) v = std::max(lower[d], std::min(v, upper[d]));
                    X[(size_t) i * n + d] = v;
                }
                strat[(size_t) j * np + i] = cauchy ? 0 : 1;
            }
        }
    }

    /* ccpso.cpp:371-435: adaptive weighting -- one weight per swarm scales its coordinates of
     * yhat; the weights are optimized by `local` inside the box that keeps yhat * w in bounds */
    void local_search()
    {
        const double inf = std::numeric_limits<double>::infinity();
        wlb.assign(nswarm, -inf);
        wub.assign(nswarm, +inf);
        wguess.assign(nswarm, 0.);
        for (int j = 0; j < nswarm; j++) {
            for (int c = 0; c < cpswarm; c++) {
                const int k = kidx[(size_t) j * cpswarm + c];
                double scale = yhat[k];
                if (std::fabs(scale) < 1e-3) scale = scale > 0. ? 1e-3 : -1e-3;
                double lbk = lower[k] / scale, ubk = upper[k] / scale;
                if (lbk > ubk) std::swap(lbk, ubk);
                wlb[j] = std::max(wlb[j], lbk);
                wub[j] = std::min(wub[j], ubk);
            }
            wguess[j] = std::max(wlb[j], std::min(1., wub[j]));
        }
        auto faux = [&](const double *w) {
            for (int j = 0; j < nswarm; j++)
                for (int c = 0; c < cpswarm; c++) {
                    const int k = kidx[(size_t) j * cpswarm + c];
                    temp[k] = yhat[k] * w[j];
                }
            return evaluate_vec(temp.data());
        };
        local->fhook = faux;
        if (rng_mode == RNG_PHILOX) {
            local->rng_mode = RNG_PHILOX;
            local->seed = local_seed0 + (uint64_t) nlocal;
        }
        nlocal++;
        if (local_fresh) {
            local->B.clear();
            local->C.clear();
        }
        local->optimize(-1, nswarm, wlb.data(), wub.data(), wguess.data());
        const std::vector<double> w(local->best_solution(), local->best_solution() + nswarm);
        fev += local->fev;
        if (correct) {
            for (int j = 0; j < nswarm; j++)
                for (int c = 0; c < cpswarm; c++) {
                    const int k = kidx[(size_t) j * cpswarm + c];
                    if (yhat[k] * w[j] < lower[k] || yhat[k] * w[j] > upper[k]) return;
                }
        }
        const double fwy = faux(w.data());
        fev++;
        if (fwy < fyhat) {
            yhat = temp;
            fyhat = fwy;
            improved = true;
        }
    }

    /* ccpso.cpp:114-122 (the reference also prints _fyhat to stdout every generation) */
    void iterate()
    {
        randomize_components();
        update_swarm();
        update_position();
        if (local && localfreq > 0 && gen % localfreq == 0) local_search();
        gen++;
    }

    bool converged()
    {
        std::vector<const double*> rows(np);
        for (int i = 0; i < np; i++) rows[i] = &X[(size_t) i * n];
        auto getx = [](const double *q) { return q; };
        if (sync) return radius_converged_sync(rows.begin(), rows.end(), getx, n, np, stol);
        return radius_converged(rows.begin(), rows.end(), getx, n, np, stol);
    }

    /* ccpso.cpp:128-148 */
    bool optimize(int obj_, int n_, const double *lo, const double *up)
    {
        init(obj_, n_, lo, up);
        while (true) {
            iterate();
            if (fev >= mfev) return false;
            if (converged()) return true;
        }
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) {
            if (cap >= 1) out[0] = v;
            return 1;
        };
        auto putv = [&](const std::vector<double> &v) {
            for (size_t q = 0; q < v.size() && (int) q < cap; q++) out[q] = v[q];
            return (int) v.size();
        };
        auto puti = [&](const std::vector<int> &v) {
            for (size_t q = 0; q < v.size() && (int) q < cap; q++) out[q] = v[q];
            return (int) v.size();
        };
        if (key == "x") return putv(X);
        if (key == "y") return putv(Y);
        if (key == "yhat") return putv(yhat);
        if (key == "fx") return putv(fX);
        if (key == "fy") return putv(fY);
        if (key == "k") return puti(kidx);
        if (key == "ibest") return puti(ibest);
        if (key == "strat") return puti(strat);
        if (key == "fyhat") return put1(fyhat);
        if (key == "phat") return put1(phat);
        if (key == "fev") return put1(fev);
        if (key == "it") return put1(gen);
        if (key == "is") return put1(is);
        if (key == "nswarm") return put1(nswarm);
        if (key == "cpswarm") return put1(cpswarm);
        if (key == "improved") return put1(improved ? 1 : 0);
        if (key == "np") return put1(np);
        return -1;
    }
};

/* ======================================================================== */
/* adaptive PSO (Zhan 2009)                                                  */
/* ======================================================================== */
struct Apso {
    int mfev = 0, np = 0;
    double tol = 0.;
    bool correct = true;
    int obj = 0, n = 0;
    std::vector<double> lower, upper, aux;
    int it = 0, fev = 0, maxit = 0, state = 0;
    double smin = 0.1, smax = 1., w = 0.9, c1 = 2., c2 = 2., vdamp = 0.2, fbest = 0.;
    std::vector<double> xbest, ws, p;
    struct Part {
        std::vector<double> x, v, xb;
        double f, fb;
    };
    std::vector<Part> swarm;
    bool sync = false;
    /* sync only: particles [k chunk, (k + 1) chunk) see the gbest as it stands after chunk k - 1
     * (0 = the whole swarm: the gbest of the generation start).  chunk = 1 is the reference's
     * in-loop refresh (apso.cpp:194-197); the device refreshes between the launches of one
     * generation (DESIGN.md "sync semantics", round 5) */
    int chunk = 0;
    int rng_mode = RNG_MT;
    uint64_t seed = 0;
    int sub = 0;
    NormalCache Z;
    double last_f = 0.;   /* evolutionary factor of the last iterate() */

    double evaluate(const double *q) { return bbo_objective_eval(obj, n, q, aux.data()); }

    /* apso.cpp:48-103 */
    void init(int obj_, int n_, const double *lo, const double *up)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        w = 0.9;
        smin = 0.1;
        smax = 1.0;
        vdamp = 0.2;
        c1 = c2 = 2.;
        state = 0;
        maxit = (int) std::round(mfev / (1. + np));
        it = 0;
        fev = 0;
        swarm.clear();
        fbest = std::numeric_limits<double>::infinity();
        xbest.assign(n, 0.);
        for (int i = 0; i < np; i++) {
            Part q;
            q.x.resize(n);
            q.v.assign(n, 0.);
            for (int j = 0; j < n; j++) {
                if (rng_mode == RNG_MT) {
                    q.x[j] = mt_uniform(lower[j], upper[j]);
                } else {
                    uint32_t ww[4];
                    bbo_philox(seed, (uint32_t) i, (uint32_t) (j >> 1), 0,
                            bbo_stream(BBO_STREAM_INIT, (uint32_t) sub), ww);
                    const double u = (j & 1) ? bbo_u01(ww[2], ww[3]) : bbo_u01(ww[0], ww[1]);
                    q.x[j] = u * (upper[j] - lower[j]) + lower[j];
                }
            }
            q.xb = q.x;
            q.f = q.fb = evaluate(q.x.data());
            fev++;
            if (q.f < fbest) {
                xbest = q.x;
                fbest = q.f;
            }
            swarm.push_back(q);
        }
        p.assign(n, 0.);
        ws.assign(np, 0.);
    }

    /* apso.cpp:300-339 */
    double getf()
    {
        double dmin = std::numeric_limits<double>::infinity();
        double dmax = -std::numeric_limits<double>::infinity();
        int ibest = 0;
        for (int i = 0; i < np; i++) {
            ws[i] = 0.;
            const double *xi = swarm[i].x.data();
            for (int j = 0; j < np; j++) {
                if (j != i) {
                    double dij = 0.;
                    const double *xj = swarm[j].x.data();
                    for (int k = 0; k < n; k++) {
                        const double dd = xi[k] - xj[k];
                        dij += dd * dd;
                    }
                    ws[i] += std::sqrt(dij);
                }
            }
            ws[i] /= (np - 1.);
            dmax = std::max(dmax, ws[i]);
            dmin = std::min(dmin, ws[i]);
            if (swarm[i].f < swarm[ibest].f) ibest = i;
        }
        if (dmax <= dmin) return 1.;
        return (ws[ibest] - dmin) / (dmax - dmin);
    }

    /* apso.cpp:387-452 */
    static double mu(double f, int i)
    {
        switch (i) {
        case 1:
            if (f >= 0. && f <= 0.4) return 0.;
            if (f > 0.4 && f <= 0.6) return 5. * f - 2.;
            if (f > 0.6 && f <= 0.7) return 1.;
            if (f > 0.7 && f <= 0.8) return -10. * f + 8.;
            return 0.;
        case 2:
            if (f >= 0. && f <= 0.2) return 0.;
            if (f > 0.2 && f <= 0.3) return 10. * f - 2.;
            if (f > 0.3 && f <= 0.4) return 1.;
            if (f > 0.4 && f <= 0.6) return -5. * f + 3.;
            return 0.;
        case 3:
            if (f >= 0. && f <= 0.1) return 1.;
            if (f > 0.1 && f <= 0.3) return -5. * f + 1.5;
            return 0.;
        default:
            if (f >= 0. && f <= 0.7) return 0.;
            if (f > 0.7 && f <= 0.9) return 5. * f - 3.5;
            return 1.;
        }
    }

    /* apso.cpp:347-385.  The rule table is indexed [r][state] with state in 1..4 on rows of
     * four entries (apso.h:48-56): an off-by-one that reads one past the row for state 4.
     * In the reference build that word is 0 (SURVEY.md Appendix A-10), restated here as an
     * explicit fifth column of zeros. */
    int next_state(double f)
    {
        static const int rule[7][5] = {
            { 1, 1, 1, 1, 0 }, { 2, 2, 2, 2, 0 }, { 3, 3, 3, 3, 0 }, { 4, 4, 4, 4, 0 },
            { 1, 2, 2, 1, 0 }, { 2, 2, 3, 3, 0 }, { 1, 1, 4, 4, 0 } };
        const double m1 = mu(f, 1), m2 = mu(f, 2), m3 = mu(f, 3), m4 = mu(f, 4);
        if (state == 0) {
            const double m[4] = { m1, m2, m3, m4 };
            int arg = 0;
            for (int i = 1; i < 4; i++)
                if (m[arg] < m[i]) arg = i;   /* std::max_element: first maximum */
            return 1 + arg;
        }
        int r;
        if (m1 > 0 && m2 > 0) r = 4;
        else if (m2 > 0 && m3 > 0) r = 5;
        else if (m1 > 0 && m4 > 0) r = 6;
        else if (m1 > 0) r = 0;
        else if (m2 > 0) r = 1;
        else if (m3 > 0) r = 2;
        else if (m4 > 0) r = 3;
        else return -1;   /* the reference throws std::invalid_argument */
        return rule[r][state];
    }

    double ctrl_uniform(int idx, double a, double b)
    {
        if (rng_mode == RNG_MT) return mt_uniform(a, b);
        uint32_t ww[4];
        bbo_philox(seed, (uint32_t) idx, 0, (uint32_t) it,
                bbo_stream(BBO_STREAM_PSO_CTRL, (uint32_t) sub), ww);
        return bbo_u01(ww[0], ww[1]) * (b - a) + a;
    }

    /* apso.cpp:200-233 */
    void update_elitist()
    {
        p = xbest;
        int d;
        double z;
        if (rng_mode == RNG_MT) {
            d = mt_int(0, n - 1);
            z = Z.draw();
        } else {
            uint32_t ww[4];
            bbo_philox(seed, 2, 0, (uint32_t) it,
                    bbo_stream(BBO_STREAM_PSO_CTRL, (uint32_t) sub), ww);
            d = bbo_uint_below(ww[0], n);
            double z1;
            bbo_normal_pair(seed, 3, 0, (uint32_t) it,
                    bbo_stream(BBO_STREAM_PSO_CTRL, (uint32_t) sub), &z, &z1);
        }
        const double sigma = smax - (smax - smin) * it / maxit;
        p[d] += (upper[d] - lower[d]) * z * sigma;
        if (correct) p[d] = std::max(lower[d], std::min(p[d], upper[d]));
        const double nu = evaluate(p.data());
        fev++;
        if (nu < fbest) {
            xbest = p;
            fbest = nu;
            return;
        }
        Part *worst = &swarm[0];
        for (auto &q : swarm)
            if (q.f > worst->f) worst = &q;
        worst->x = p;
        worst->f = nu;
        if (nu < worst->fb) {
            worst->xb = worst->x;
            worst->fb = nu;
        }
    }

    /* apso.cpp:248-298 */
    void update_c1c2(double f, int st)
    {
        w = 1. / (1. + 1.5 * std::exp(-2.6 * f));
        const double delta1 = ctrl_uniform(0, 0.05, 0.1);
        const double delta2 = ctrl_uniform(1, 0.05, 0.1);
        switch (st) {
        case 1: c1 += delta1; c2 -= delta2; break;
        case 2: c1 += 0.5 * delta1; c2 -= 0.5 * delta2; break;
        case 3: c1 += 0.5 * delta1; c2 += 0.5 * delta2; update_elitist(); break;
        default: c1 -= 0.5 * delta1; c2 += 0.5 * delta2; break;
        }
        c1 = std::max(1.5, std::min(c1, 2.5));
        c2 = std::max(1.5, std::min(c2, 2.5));
        if (c1 + c2 > 4.) {
            const double fac = 4. / (c1 + c2);
            c1 *= fac;
            c2 *= fac;
        }
    }

    /* apso.cpp:159-198; sync: every particle sees the gbest of the generation start -- or, with
     * chunk > 0, of the start of its chunk */
    void update_swarm()
    {
        std::vector<double> gb = xbest;
        const double *g = sync ? gb.data() : xbest.data();
        double fmin = fbest;
        int imin = -1;
        for (int i = 0; i < np; i++) {
            if (sync && chunk > 0 && i > 0 && i % chunk == 0) {
                if (imin >= 0) {
                    xbest = swarm[imin].x;
                    fbest = fmin;
                    imin = -1;
                }
                gb = xbest;
            }
            Part &q = swarm[i];
            for (int j = 0; j < n; j++) {
                double r1, r2;
                if (rng_mode == RNG_MT) {
                    r1 = mt_uniform(0., 1.);
                    r2 = mt_uniform(0., 1.);
                } else {
                    uint32_t ww[4];
                    bbo_philox(seed, (uint32_t) i, (uint32_t) j, (uint32_t) it,
                            bbo_stream(BBO_STREAM_PSO_R, (uint32_t) sub), ww);
                    r1 = bbo_u01(ww[0], ww[1]);
                    r2 = bbo_u01(ww[2], ww[3]);
                }
                q.v[j] = q.v[j] * w + c1 * r1 * (q.xb[j] - q.x[j]) + c2 * r2 * (g[j] - q.x[j]);
                const double vmax = vdamp * (upper[j] - lower[j]);
                q.v[j] = std::max(-vmax, std::min(q.v[j], vmax));
                q.x[j] += q.v[j];
            }
            if (correct)
                for (int j = 0; j < n; j++) q.x[j] = std::max(lower[j], std::min(q.x[j], upper[j]));
            q.f = evaluate(q.x.data());
            fev++;
            if (q.f < q.fb) {
                q.xb = q.x;
                q.fb = q.f;
            }
            if (!sync) {
                if (q.f < fbest) {
                    xbest = q.x;
                    fbest = q.f;
                }
            } else if (q.f < fmin) {
                fmin = q.f;
                imin = i;
            }
        }
        if (sync && imin >= 0) {
            xbest = swarm[imin].x;
            fbest = fmin;
        }
    }

    int iterate()
    {
        const double f = getf();
        last_f = f;
        const int ns = next_state(f);
        if (ns < 0) return -1;
        update_c1c2(f, ns);
        state = ns;
        update_swarm();
        it++;
        return 0;
    }

    bool converged()
    {
        auto getx = [](const Part &q) { return q.x.data(); };
        if (sync) return radius_converged_sync(swarm.begin(), swarm.end(), getx, n, np, tol);
        return radius_converged(swarm.begin(), swarm.end(), getx, n, np, tol);
    }

    bool optimize(int obj_, int n_, const double *lo, const double *up)
    {
        init(obj_, n_, lo, up);
        while (it < maxit && fev < mfev) {
            iterate();
            if (converged()) return true;
        }
        return false;
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) { if (cap > 0) out[0] = v; return 1; };
        if (key == "x" || key == "v" || key == "xb") {
            int m = 0;
            for (const auto &q : swarm) {
                const auto &src = key == "x" ? q.x : key == "v" ? q.v : q.xb;
                for (double v : src) {
                    if (m < cap) out[m] = v;
                    m++;
                }
            }
            return m;
        }
        if (key == "f" || key == "fb") {
            int m = 0;
            for (const auto &q : swarm) {
                if (m < cap) out[m] = key == "f" ? q.f : q.fb;
                m++;
            }
            return m;
        }
        if (key == "xbest") {
            for (int i = 0; i < n && i < cap; i++) out[i] = xbest[i];
            return n;
        }
        if (key == "ws") {
            for (int i = 0; i < np && i < cap; i++) out[i] = ws[i];
            return np;
        }
        if (key == "fbest") return put1(fbest);
        if (key == "w") return put1(w);
        if (key == "c1") return put1(c1);
        if (key == "c2") return put1(c2);
        if (key == "state") return put1(state);
        if (key == "it") return put1(it);
        if (key == "maxit") return put1(maxit);
        if (key == "fev") return put1(fev);
        if (key == "np") return put1(np);
        if (key == "evof") return put1(last_f);
        return -1;
    }
};

/* ======================================================================== */
/* restart drivers over a borrowed Cma                                       */
/* ======================================================================== */
struct Restart {
    int kind = 1;   /* 0 = IPOP (ipop_cmaes.cpp), 1 = BIPOP (bipop_cmaes.cpp) */
    Cma *base = nullptr;
    /* parameters */
    int mfev = 0, maxlargeruns = 9;
    double sigmadef = 2., ksigmadec = 1.6, kbudget = 2.;
    bool nflag = true;        /* nipop / nbipop */
    bool boundlambda = true;
    /* problem */
    int obj = 0, n = 0;
    std::vector<double> lower, upper, guess, x0, xbest, aux;
    /* state */
    int fev = 0, it = 0, lambdadef = 0, lambda = 0, lambdamax = 0;
    int largelambda = 0, smalllambda = 0, largebudget = 0, smallbudget = 0;
    int largerestarts = 0, smallrestarts = 0, bestregime = 1;
    double fx = 0., fxbest = 0., sigma = 0., largesigma = 0., smallsigma = 0.;
    int last_regime = 0, last_inner_fev = 0, last_lambda = 0, last_maxfev = 0;
    double last_sigma = 0.;
    /* randomness of the driver itself (restart points, u, u') */
    int rng_mode = RNG_MT;
    uint64_t seed = 0;

    double evaluate(const double *q) { return bbo_objective_eval(obj, n, q, aux.data()); }

    /* k: draw index inside run it + 1 (coordinates 0..n-1, then u, u'); the mt19937 mode
     * consumes the global stream in call order like the reference and ignores it */
    double uniform(int k, double a, double b)
    {
        if (rng_mode == RNG_MT) return mt_uniform(a, b);
        uint32_t w[4];
        bbo_philox(seed, (uint32_t) (it + 1), (uint32_t) k, 0, bbo_stream(BBO_STREAM_RESTART, 0), w);
        return bbo_u01(w[0], w[1]) * (b - a) + a;
    }

    /* bipop_cmaes.cpp:191-202 == ipop_cmaes.cpp:178-189 */
    int max_evaluations(int lam) const
    {
        const int maxit = (int) (100. + 50. * (n + 3) * (n + 3) / std::sqrt(1. * lam));
        return std::min(maxit * lam, mfev - fev);
    }

    /* one inner run: setParams + optimize + the extra evaluation (bipop_cmaes.cpp:83-87) */
    int inner(int lam, double sig, int maxfev, const double *start)
    {
        base->set_params(lam, sig, maxfev);
        last_maxfev = maxfev;
        if (rng_mode != RNG_MT) base->seed = seed + 0x9E3779B97F4A7C15ull * (uint64_t) (it + 1);
        base->optimize(obj, n, lower.data(), upper.data(), start);
        const double *xb = base->best_solution();
        std::vector<double> x(xb, xb + n);
        fx = evaluate(x.data());
        fev += base->fev + 1;
        last_inner_fev = base->fev;
        last_lambda = lam;
        last_sigma = sig;
        if (it < 0 || fx < fxbest) {
            fxbest = fx;
            xbest = x;
            return 1;
        }
        return 0;
    }

    void init(int obj_, int n_, const double *lo, const double *up, const double *g)
    {
        obj = obj_;
        n = n_;
        lower.assign(lo, lo + n);
        upper.assign(up, up + n);
        guess.assign(g, g + n);
        aux.assign(n, 0.);
        bbo_objective_aux(obj, n, aux.data());
        fev = 0;
        lambda = lambdadef = 4 + (int) (3. * std::log(1. * n));
        lambdamax = 10 * n * n;
        sigma = sigmadef;
        const int maxfev = max_evaluations(lambdadef);
        it = -1;   /* marks "first run": always becomes the incumbent */
        inner(lambdadef, sigmadef, maxfev, guess.data());
        largebudget = smallbudget = 0;
        largerestarts = smallrestarts = 0;
        bestregime = 1;
        it = 0;
        x0.assign(n, 0.);
        last_regime = 0;
    }

    /* ipop_cmaes.cpp:112-162 */
    void iterate_ipop()
    {
        for (int i = 0; i < n; i++) x0[i] = uniform(i, lower[i], upper[i]);
        if (boundlambda) {
            lambda <<= 1;
            if (lambda > lambdamax) {
                if (lambda - lambdamax < lambdamax - (lambda >> 1)) lambda = lambdamax;
                else lambda = lambdadef;
            }
        } else {
            lambda <<= 1;
        }
        if (nflag) {
            sigma /= ksigmadec;
            sigma = std::max(sigma, 0.01 * sigmadef);
        }
        const int maxfev = max_evaluations(lambda);
        inner(lambda, sigma, maxfev, x0.data());
        it++;
    }

    /* bipop_cmaes.cpp:109-164, :204-267 */
    void iterate_bipop()
    {
        for (int i = 0; i < n; i++) x0[i] = uniform(i, lower[i], upper[i]);
        int regime;
        if (nflag) {
            if (bestregime == 1) regime = (largebudget <= smallbudget * kbudget) ? 1 : 2;
            else regime = (smallbudget <= kbudget * largebudget) ? 2 : 1;
        } else {
            regime = (largebudget <= smallbudget) ? 1 : 2;
        }
        if (regime == 1) {
            largelambda = (int) (lambdadef * std::pow(2, largerestarts + 1));
            if (nflag) {
                largesigma = sigmadef * std::pow(1. / ksigmadec, largerestarts + 1);
                largesigma = std::max(largesigma, 0.01 * sigmadef);
            } else {
                largesigma = sigmadef;
            }
            const int maxfev = max_evaluations(largelambda);
            if (inner(largelambda, largesigma, maxfev, x0.data())) bestregime = 1;
            largebudget += last_inner_fev;
            largerestarts++;
        } else {
            const double u = uniform(n, 0., 1.);
            smalllambda = (int) (lambdadef * std::pow((0.5 * largelambda) / lambdadef, u * u));
            smallsigma = sigmadef * std::pow(10., -2. * uniform(n + 1, 0., 1.));
            int maxfev = max_evaluations(smalllambda);
            maxfev = std::min(maxfev, largebudget >> 1);
            if (inner(smalllambda, smallsigma, maxfev, x0.data())) bestregime = 2;
            smallbudget += last_inner_fev;
            smallrestarts++;
        }
        last_regime = regime;
        it++;
    }

    void iterate()
    {
        if (kind == 0) iterate_ipop();
        else iterate_bipop();
    }

    void optimize(int obj_, int n_, const double *lo, const double *up, const double *g)
    {
        init(obj_, n_, lo, up, g);
        if (kind == 0) {
            while (fev < mfev) iterate();
        } else {
            while (true) {
                iterate();
                if (largerestarts >= maxlargeruns) break;
                if (fev >= mfev) break;
            }
        }
    }

    int get(const std::string &key, double *out, int cap)
    {
        auto put1 = [&](double v) { if (cap > 0) out[0] = v; return 1; };
        if (key == "xbest" || key == "x0") {
            const auto &v = key == "xbest" ? xbest : x0;
            for (size_t i = 0; i < v.size() && (int) i < cap; i++) out[i] = v[i];
            return (int) v.size();
        }
        if (key == "fev") return put1(fev);
        if (key == "it") return put1(it);
        if (key == "lambdadef") return put1(lambdadef);
        if (key == "lambda") return put1(lambda);
        if (key == "sigma") return put1(sigma);
        if (key == "largelambda") return put1(largelambda);
        if (key == "smalllambda") return put1(smalllambda);
        if (key == "largebudget") return put1(largebudget);
        if (key == "smallbudget") return put1(smallbudget);
        if (key == "largerestarts") return put1(largerestarts);
        if (key == "smallrestarts") return put1(smallrestarts);
        if (key == "bestregime") return put1(bestregime);
        if (key == "fx") return put1(fx);
        if (key == "fxbest" || key == "fbest") return put1(fxbest);
        if (key == "largesigma") return put1(largesigma);
        if (key == "smallsigma") return put1(smallsigma);
        if (key == "last_regime") return put1(last_regime);
        if (key == "last_lambda") return put1(last_lambda);
        if (key == "last_sigma") return put1(last_sigma);
        if (key == "last_inner_fev") return put1(last_inner_fev);
        if (key == "last_maxfev") return put1(last_maxfev);
        return -1;
    }

    /* test support: the driver's bookkeeping taken over from another implementation's history,
     * so that the NEXT decision (bipop_cmaes.cpp:109-142, ipop_cmaes.cpp:112-135) can be
     * compared on its own */
    int set(const std::string &key, double v)
    {
        if (key == "fev") fev = (int) v;
        else if (key == "it") it = (int) v;
        else if (key == "lambda") lambda = (int) v;
        else if (key == "sigma") sigma = v;
        else if (key == "largelambda") largelambda = (int) v;
        else if (key == "largebudget") largebudget = (int) v;
        else if (key == "smallbudget") smallbudget = (int) v;
        else if (key == "largerestarts") largerestarts = (int) v;
        else if (key == "smallrestarts") smallrestarts = (int) v;
        else if (key == "bestregime") bestregime = (int) v;
        else if (key == "fxbest") fxbest = v;
        else return -1;
        return 1;
    }
};

} // namespace

extern "C" {

/* ---- L-SHADE / JADE ------------------------------------------------------- */
void* orc_shade_create(int mfev, int npinit, double tol, int archive, int repaircr, int h,
        int npmin)
{
    De *d = new De();
    d->variant = 0;
    d->mfev = mfev;
    d->npinit = npinit;
    d->tol = tol;
    d->archive = archive != 0;
    d->repaircr = repaircr != 0;
    d->h = h;
    d->npmin = npmin;
    return d;
}
void* orc_jade_create(int mfev, int np, double tol, int archive, int repaircr, double pelite,
        double cdamp, double sigma)
{
    De *d = new De();
    d->variant = 1;
    d->mfev = mfev;
    d->npinit = np;
    d->npmin = np;
    d->tol = tol;
    d->archive = archive != 0;
    d->repaircr = repaircr != 0;
    d->pelite = pelite;
    d->cdamp = cdamp;
    d->jsigma = sigma;
    d->h = 1;
    return d;
}
#define ORC_DE_API(NAME)                                                               \
void orc_##NAME##_destroy(void *p) { delete static_cast<De*>(p); }                    \
void orc_##NAME##_init(void *p, int obj, int n, const double *lo, const double *up,  \
        const double *guess)                                                           \
{                                                                                      \
    (void) guess;   /* ignored by the reference too (SURVEY.md Appendix A-16) */      \
    static_cast<De*>(p)->init(obj, n, lo, up);                                         \
}                                                                                      \
void orc_##NAME##_iterate(void *p) { static_cast<De*>(p)->iterate(); }                \
int orc_##NAME##_get(void *p, const char *key, double *out, int cap)                  \
{                                                                                      \
    return static_cast<De*>(p)->get(key, out, cap);                                    \
}                                                                                      \
void orc_##NAME##_solution(void *p, double *x, int *fev, int *conv)                   \
{                                                                                      \
    De *d = static_cast<De*>(p);                                                       \
    d->sort_swarm();                                                                   \
    for (int i = 0; i < d->n; i++) x[i] = d->swarm[0].x[i];                            \
    *fev = d->fev;                                                                     \
    *conv = d->converged() ? 1 : 0;                                                    \
}                                                                                      \
int orc_##NAME##_optimize(void *p, int obj, int n, const double *lo, const double *up,\
        const double *guess, double *x, int *fev, int *conv)                           \
{                                                                                      \
    (void) guess;                                                                      \
    De *d = static_cast<De*>(p);                                                       \
    const bool c = d->optimize(obj, n, lo, up);                                        \
    for (int i = 0; i < n; i++) x[i] = d->swarm[0].x[i];                               \
    *fev = d->fev;                                                                     \
    *conv = c ? 1 : 0;                                                                 \
    return 0;                                                                          \
}
ORC_DE_API(shade)
ORC_DE_API(jade)

/* ---- APSO -------------------------------------------------------------------- */
void* orc_apso_create(int mfev, double tol, int np, int correct)
{
    Apso *a = new Apso();
    a->mfev = mfev;
    a->tol = tol;
    a->np = np;
    a->correct = correct != 0;
    return a;
}
void orc_apso_destroy(void *p) { delete static_cast<Apso*>(p); }
void orc_apso_init(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess)
{
    (void) guess;
    static_cast<Apso*>(p)->init(obj, n, lo, up);
}
void orc_apso_iterate(void *p) { static_cast<Apso*>(p)->iterate(); }
int orc_apso_get(void *p, const char *key, double *out, int cap)
{
    return static_cast<Apso*>(p)->get(key, out, cap);
}
void orc_apso_solution(void *p, double *x, int *fev, int *conv)
{
    Apso *a = static_cast<Apso*>(p);
    for (int i = 0; i < a->n; i++) x[i] = a->xbest[i];
    *fev = a->fev;
    *conv = a->converged() ? 1 : 0;
}
int orc_apso_optimize(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess, double *x, int *fev, int *conv)
{
    (void) guess;
    Apso *a = static_cast<Apso*>(p);
    const bool c = a->optimize(obj, n, lo, up);
    for (int i = 0; i < n; i++) x[i] = a->xbest[i];
    *fev = a->fev;
    *conv = c ? 1 : 0;
    return 0;
}

/* ---- SaNSDE ---------------------------------------------------------------------- */
void* orc_sansde_create(int mfev, int np, double tol, int repaircr, int crref, int pupdate,
        int crupdate)
{
    Sansde *d = new Sansde();
    d->mfev = mfev;
    d->np = np;
    d->tol = tol;
    d->repaircr = repaircr != 0;
    d->ncrref = crref;
    d->npup = pupdate;
    d->ncrup = crupdate;
    return d;
}
void orc_sansde_destroy(void *p) { delete static_cast<Sansde*>(p); }
void orc_sansde_init(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess)
{
    (void) guess;
    static_cast<Sansde*>(p)->init(obj, n, lo, up);
}
void orc_sansde_iterate(void *p) { static_cast<Sansde*>(p)->iterate(); }
int orc_sansde_get(void *p, const char *key, double *out, int cap)
{
    return static_cast<Sansde*>(p)->get(key, out, cap);
}
void orc_sansde_solution(void *p, double *x, int *fev, int *conv)
{
    Sansde *d = static_cast<Sansde*>(p);
    d->sort_swarm();
    for (int i = 0; i < d->n; i++) x[i] = d->swarm[0].x[i];
    *fev = d->fev;
    *conv = d->converged() ? 1 : 0;
}
int orc_sansde_optimize(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess, double *x, int *fev, int *conv)
{
    (void) guess;
    Sansde *d = static_cast<Sansde*>(p);
    const bool c = d->optimize(obj, n, lo, up);
    for (int i = 0; i < n; i++) x[i] = d->swarm[0].x[i];
    *fev = d->fev;
    *conv = c ? 1 : 0;
    return 0;
}

/* ---- CSO -------------------------------------------------------------------------- */
void* orc_cso_create(int mfev, double stol, int np, int pcompete, int ring, int correct,
        double vmax)
{
    Cso *c = new Cso();
    c->mfev = mfev;
    c->stol = stol;
    c->np = np;
    c->pcompete = pcompete;
    c->ring = ring != 0;
    c->correct = correct != 0;
    c->vmax = vmax;
    c->configure();
    return c;
}
void orc_cso_destroy(void *p) { delete static_cast<Cso*>(p); }
void orc_cso_init(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess)
{
    (void) guess;
    static_cast<Cso*>(p)->init(obj, n, lo, up);
}
void orc_cso_iterate(void *p) { static_cast<Cso*>(p)->iterate(); }
int orc_cso_get(void *p, const char *key, double *out, int cap)
{
    return static_cast<Cso*>(p)->get(key, out, cap);
}
void orc_cso_solution(void *p, double *x, int *fev, int *conv)
{
    Cso *c = static_cast<Cso*>(p);
    for (int i = 0; i < c->n; i++) x[i] = c->swarm[c->ibest].x[i];
    *fev = c->fev;
    *conv = c->converged() ? 1 : 0;
}
int orc_cso_optimize(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess, double *x, int *fev, int *conv)
{
    (void) guess;
    Cso *c = static_cast<Cso*>(p);
    const bool cv = c->optimize(obj, n, lo, up);
    for (int i = 0; i < n; i++) x[i] = c->swarm[c->ibest].x[i];
    *fev = c->fev;
    *conv = cv ? 1 : 0;
    return 0;
}

/* ---- CCPSO ------------------------------------------------------------------------ */
void* orc_ccpso_create(int mfev, double stol, int np, const int *pps, int npps, int correct,
        double pcauchy)
{
    Ccpso *c = new Ccpso();
    c->mfev = mfev;
    c->stol = stol;
    c->np = np;
    c->pps.assign(pps, pps + npps);
    c->correct = correct != 0;
    c->phat0 = pcauchy;
    return c;
}
void orc_ccpso_destroy(void *p) { delete static_cast<Ccpso*>(p); }
/* takes ownership of `cma` (an orc_cma_create handle); local_seed: Philox mode only */
void orc_ccpso_set_local(void *p, void *cma, int localfreq, uint64_t local_seed)
{
    Ccpso *h = static_cast<Ccpso*>(p);
    delete h->local;
    h->local = static_cast<Cma*>(cma);
    h->localfreq = localfreq;
    h->local_seed0 = local_seed;
}
void orc_ccpso_local_fresh(void *p, int fresh) { static_cast<Ccpso*>(p)->local_fresh = fresh != 0; }
void orc_ccpso_init(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess)
{
    (void) guess;
    static_cast<Ccpso*>(p)->init(obj, n, lo, up);
}
void orc_ccpso_iterate(void *p) { static_cast<Ccpso*>(p)->iterate(); }
void orc_ccpso_set_shard(void *p, int rank, int world)
{
    Ccpso *c = static_cast<Ccpso*>(p);
    c->shard_rank = rank;
    c->shard_world = world;
}
void orc_ccpso_phase(void *p, int which) { static_cast<Ccpso*>(p)->phase(which); }
int orc_ccpso_table_record(void *p)
{
    Ccpso *c = static_cast<Ccpso*>(p);
    return 2 * c->n * c->np;
}
void orc_ccpso_export_tables(void *p, double *out) { static_cast<Ccpso*>(p)->export_tables(out); }
void orc_ccpso_merge_tables(void *p, const double *g, int world)
{
    static_cast<Ccpso*>(p)->merge_tables(g, world);
}
int orc_ccpso_get(void *p, const char *key, double *out, int cap)
{
    return static_cast<Ccpso*>(p)->get(key, out, cap);
}
void orc_ccpso_solution(void *p, double *x, int *fev, int *conv)
{
    Ccpso *c = static_cast<Ccpso*>(p);
    for (int i = 0; i < c->n; i++) x[i] = c->yhat[i];
    *fev = c->fev;
    *conv = c->converged() ? 1 : 0;
}
int orc_ccpso_optimize(void *p, int obj, int n, const double *lo, const double *up,
        const double *guess, double *x, int *fev, int *conv)
{
    (void) guess;
    Ccpso *c = static_cast<Ccpso*>(p);
    const bool cv = c->optimize(obj, n, lo, up);
    for (int i = 0; i < n; i++) x[i] = c->yhat[i];
    *fev = c->fev;
    *conv = cv ? 1 : 0;
    return 0;
}

/* sync / generator selection for SHADE, JADE, APSO handles (kind: 0 DE, 1 APSO) */
void orc_pop_set_mode(void *p, int kind, int sync, int rng_mode, uint64_t seed)
{
    if (kind == 0) {
        De *d = static_cast<De*>(p);
        d->sync = sync != 0;
        d->rng_mode = rng_mode;
        d->seed = seed;
    } else if (kind == 4) {
        Ccpso *c = static_cast<Ccpso*>(p);
        c->sync = sync != 0;
        c->rng_mode = rng_mode;
        c->seed = seed;
    } else if (kind == 3) {
        Cso *c = static_cast<Cso*>(p);
        c->sync = sync != 0;
        c->rng_mode = rng_mode;
        c->seed = seed;
    } else if (kind == 2) {
        Sansde *d = static_cast<Sansde*>(p);
        d->sync = sync != 0;
        d->rng_mode = rng_mode;
        d->seed = seed;
    } else {
        Apso *a = static_cast<Apso*>(p);
        a->sync = sync != 0;
        a->rng_mode = rng_mode;
        a->seed = seed;
    }
}

/* Philox sub-stream of a Philox-mode handle (same `kind` as orc_pop_set_mode): object `sub` draws
 * what population `sub` of a batched device handle draws.  Call before init. */
void orc_pop_set_sub(void *p, int kind, int sub)
{
    if (kind == 0) static_cast<De*>(p)->sub = sub;
    else if (kind == 4) static_cast<Ccpso*>(p)->sub = sub;
    else if (kind == 3) static_cast<Cso*>(p)->sub = sub;
    else if (kind == 2) static_cast<Sansde*>(p)->sub = sub;
    else static_cast<Apso*>(p)->sub = sub;
}

void orc_apso_set_chunk(void *p, int chunk) { static_cast<Apso*>(p)->chunk = chunk; }

/* ---- restart drivers ------------------------------------------------------------ */
void* orc_bipop_create(void *base, int mfev, double sigma0, int maxlargeruns, int nbipop,
        double ksigmadec, double kbudget)
{
    Restart *r = new Restart();
    r->kind = 1;
    r->base = static_cast<Cma*>(base);   /* takes ownership, like the harness */
    r->mfev = mfev;
    r->sigmadef = sigma0;
    r->maxlargeruns = maxlargeruns;
    r->nflag = nbipop != 0;
    r->ksigmadec = ksigmadec;
    r->kbudget = kbudget;
    return r;
}
void* orc_ipop_create(void *base, int mfev, double sigma0, int nipop, double ksigmadec,
        int boundlambda)
{
    Restart *r = new Restart();
    r->kind = 0;
    r->base = static_cast<Cma*>(base);
    r->mfev = mfev;
    r->sigmadef = sigma0;
    r->nflag = nipop != 0;
    r->ksigmadec = ksigmadec;
    r->boundlambda = boundlambda != 0;
    return r;
}
#define ORC_RESTART_API(NAME)                                                          \
void orc_##NAME##_destroy(void *p)                                                     \
{                                                                                      \
    Restart *r = static_cast<Restart*>(p);                                             \
    delete r->base;                                                                    \
    delete r;                                                                          \
}                                                                                      \
void orc_##NAME##_init(void *p, int obj, int n, const double *lo, const double *up,  \
        const double *guess)                                                           \
{                                                                                      \
    static_cast<Restart*>(p)->init(obj, n, lo, up, guess);                             \
}                                                                                      \
void orc_##NAME##_iterate(void *p) { static_cast<Restart*>(p)->iterate(); }           \
int orc_##NAME##_get(void *p, const char *key, double *out, int cap)                  \
{                                                                                      \
    return static_cast<Restart*>(p)->get(key, out, cap);                               \
}                                                                                      \
int orc_##NAME##_optimize(void *p, int obj, int n, const double *lo, const double *up,\
        const double *guess, double *x, int *fev, int *conv)                           \
{                                                                                      \
    Restart *r = static_cast<Restart*>(p);                                             \
    r->optimize(obj, n, lo, up, guess);                                                \
    for (int i = 0; i < n; i++) x[i] = r->xbest[i];                                    \
    *fev = r->fev;                                                                     \
    *conv = 0;                                                                         \
    return 0;                                                                          \
}
ORC_RESTART_API(bipop)
ORC_RESTART_API(ipop)
int orc_bipop_inner_get(void *p, const char *key, double *out, int cap)
{
    return static_cast<Restart*>(p)->base->get(key, out, cap);
}
int orc_restart_set(void *p, const char *key, double v)
{
    return static_cast<Restart*>(p)->set(key, v);
}
void orc_restart_set_rng(void *p, int rng_mode, uint64_t seed)
{
    Restart *r = static_cast<Restart*>(p);
    r->rng_mode = rng_mode;
    r->seed = seed;
    r->base->rng_mode = rng_mode;
}

} // extern "C"
