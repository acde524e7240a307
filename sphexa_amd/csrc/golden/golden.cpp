/*! Golden-value harness: the SPH j-loops of sph_math.hpp instantiated in double precision (-DSPHX_HYDRO_TYPE=double),
 *  as the reference pins its kernels with T = double in sph/test/ve.cpp:112-232 and sph/test/std.cpp:98-123.
 *
 *  Every entry point evaluates particle 0 of the given arrays against the neighbor list 1..n-1 (the reference
 *  fixture layout) through the same SoA loaders the OpenMP path uses, and returns the loop outputs. The production
 *  fp32 paths (OpenMP and gfx950) are pinned to the same fixture through the regular operators (tests/test_golden.py).
 *
 *  The ``*_all`` entry points evaluate every particle of the arrays against its own neighbor list (CSR: int64 offsets,
 *  int32 indices, self excluded) in a box given as lo[3], hi[3], bc[3], for any kernel choice and sinc index (the tables
 *  come from the caller): the all-particle fp64 oracle of tests/test_pairloop_oracle.py.
 */
#include <initializer_list>
#include <numeric>
#include <stdexcept>
#include <vector>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "sphx/sph_math.hpp"

namespace py = pybind11;
using namespace sphx;

static_assert(sizeof(HT) == 8, "the golden harness is built with -DSPHX_HYDRO_TYPE=double");

using Arr = py::array_t<double, py::array::c_style | py::array::forcecast>;

namespace
{

const double* ptr(const Arr& a) { return a.data(); }

struct Fixture
{
    std::vector<int32_t> nbr;
    unsigned nc;
    explicit Fixture(size_t n)
        : nbr(n - 1)
        , nc(unsigned(n - 1))
    {
        std::iota(nbr.begin(), nbr.end(), 1);
    }
};

Box openBox(double lo, double hi)
{
    Box b;
    for (int d = 0; d < 3; ++d)
    {
        b.lo[d] = lo;
        b.hi[d] = hi;
        b.bc[d] = 0;
    }
    return b;
}

KernelFn kernel(const Arr& wh, const Arr& whd, double sincIndex, int choice = 0)
{
    return KernelFn{ptr(wh), ptr(whd), sincIndex, choice};
}

using Vec3  = std::vector<double>;
using IdxArr = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using OffArr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;

Box boxOf(const Vec3& lo, const Vec3& hi, const std::vector<int>& bc)
{
    if (lo.size() != 3 || hi.size() != 3 || bc.size() != 3) throw std::invalid_argument("box: lo[3], hi[3], bc[3]");
    Box b;
    for (int d = 0; d < 3; ++d)
    {
        b.lo[d] = lo[d];
        b.hi[d] = hi[d];
        b.bc[d] = bc[d];
    }
    return b;
}

//! @brief CSR neighbor lists of all targets: list of i is idx[off[i] .. off[i+1])
struct Csr
{
    const int64_t* off;
    const int32_t* idx;
    size_t n;
    Csr(const OffArr& o, const IdxArr& k, size_t n_)
        : off(o.data())
        , idx(k.data())
        , n(n_)
    {
        if (size_t(o.size()) != n + 1 || o.data()[0] != 0 || o.data()[n] != int64_t(k.size()))
            throw std::invalid_argument("CSR offsets do not match the particle and index counts");
        for (size_t i = 0; i < n; ++i)
            if (o.data()[i + 1] < o.data()[i]) throw std::invalid_argument("CSR offsets decrease");
        for (py::ssize_t q = 0; q < k.size(); ++q)
            if (k.data()[q] < 0 || size_t(k.data()[q]) >= n) throw std::invalid_argument("neighbor index out of range");
    }
    const int32_t* list(size_t i) const { return idx + off[i]; }
    unsigned count(size_t i) const { return unsigned(off[i + 1] - off[i]); }
};

void sameSize(size_t n, std::initializer_list<const Arr*> as)
{
    for (const Arr* a : as)
        if (size_t(a->size()) != n) throw std::invalid_argument("particle arrays differ in size");
}

py::array_t<double> out1(size_t n) { return py::array_t<double>(py::ssize_t(n)); }
py::array_t<double> out6(size_t n) { return py::array_t<double>({py::ssize_t(6), py::ssize_t(n)}); }

//! @brief the six rows of a (6, n) array
struct Rows6
{
    const double* r[6];
    Rows6(const Arr& a, size_t n)
    {
        if (a.ndim() != 2 || a.shape(0) != 6 || size_t(a.shape(1)) != n) throw std::invalid_argument("expected (6, n)");
        for (int k = 0; k < 6; ++k)
            r[k] = a.data() + size_t(k) * n;
    }
};

} // namespace

PYBIND11_MODULE(_sphx_golden, m)
{
    m.doc() = "fp64 instantiation of the SPH j-loops for golden-value tests";

    m.def("xmass", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr h, Arr mass, Arr wh, Arr whd,
                      double n) {
        Fixture f(x.size());
        SoaPos ld{ptr(x), ptr(y), ptr(z), ptr(mass), nullptr};
        return xmassJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ptr(h)[0], ld, kernel(wh, whd, n));
    });

    m.def("ve_def_gradh", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr h, Arr mass, Arr xm, Arr wh,
                             Arr whd, double n) {
        Fixture f(x.size());
        SoaPos ld{ptr(x), ptr(y), ptr(z), ptr(mass), ptr(xm)};
        HT kx, gradh;
        veDefGradhJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ptr(h)[0], ld, kernel(wh, whd, n), kx, gradh);
        return py::make_tuple(kx, gradh);
    });

    m.def("iad", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr h, Arr numer, Arr denom, Arr wh, Arr whd,
                    double n) {
        Fixture f(x.size());
        SoaIad ld{ptr(x), ptr(y), ptr(z), ptr(numer), ptr(denom), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        HT c[6];
        iadJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ptr(h)[0], ld, kernel(wh, whd, n), c);
        return std::vector<double>(c, c + 6);
    });

    m.def("divv_curlv", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr vx, Arr vy, Arr vz, Arr h,
                           std::vector<double> ci, Arr kx, Arr xm, Arr wh, Arr whd, double n) {
        Fixture f(x.size());
        SoaIad ld{ptr(x), ptr(y), ptr(z), nullptr, nullptr, ptr(vx), ptr(vy), ptr(vz), ptr(xm), nullptr, nullptr};
        HT divv, curlv, dV[6];
        divvCurlvJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ptr(h)[0], ptr(kx)[0], ci.data(), ld,
                       kernel(wh, whd, n), divv, curlv, dV);
        return py::make_tuple(divv, curlv, std::vector<double>(dV, dV + 6));
    });

    m.def("av_switches", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr vx, Arr vy, Arr vz, Arr h, Arr c,
                            std::vector<double> ci, Arr kx, Arr xm, Arr divv, Arr wh, Arr whd, double n, double dt,
                            double alphamin, double alphamax, double decay, double alpha0) {
        Fixture f(x.size());
        SoaIad ld{ptr(x), ptr(y), ptr(z), ptr(xm), ptr(kx), ptr(vx), ptr(vy), ptr(vz), nullptr, ptr(c), ptr(divv)};
        return avSwitchesJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ptr(h)[0], ci.data(), ld,
                               kernel(wh, whd, n), dt, alphamin, alphamax, decay, alpha0);
    });

    m.def("momentum_energy", [](bool avClean, double K, double Atmin, double Atmax, double lo, double hi, Arr x, Arr y,
                                Arr z, Arr vx, Arr vy, Arr vz, Arr h, Arr c11, Arr c12, Arr c13, Arr c22, Arr c23,
                                Arr c33, Arr mass, Arr c, Arr xm, Arr kx, Arr prho, Arr alpha, std::vector<Arr> dV,
                                Arr wh, Arr whd, double n) {
        Fixture f(x.size());
        SphConsts sc{};
        sc.K     = K;
        sc.Atmin = float(Atmin);
        sc.Atmax = float(Atmax);
        sc.ramp  = float(1.0 / (Atmax - Atmin));
        SoaMom ld{ptr(x),   ptr(y),   ptr(z),   ptr(vx),  ptr(vy),   ptr(vz), ptr(h),  ptr(c11), ptr(c12), ptr(c13),
                  ptr(c22), ptr(c23), ptr(c33), ptr(mass), ptr(c),   ptr(xm), ptr(kx), ptr(prho), ptr(alpha)};
        SoaGradV ldg{{ptr(dV[0]), ptr(dV[1]), ptr(dV[2]), ptr(dV[3]), ptr(dV[4]), ptr(dV[5])}};
        HT ax, ay, az, maxvs;
        double du;
        Box box = openBox(lo, hi);
        KernelFn kf = kernel(wh, whd, n);
        if (avClean)
            momentumEnergyJLoop<true>(0, sc, box, f.nbr.data(), 1, f.nc, ld, ldg, kf, ax, ay, az, du, maxvs);
        else
            momentumEnergyJLoop<false>(0, sc, box, f.nbr.data(), 1, f.nc, ld, ldg, kf, ax, ay, az, du, maxvs);
        return py::make_tuple(ax, ay, az, du, maxvs);
    });

    m.def("momentum_energy_std", [](double K, double lo, double hi, Arr x, Arr y, Arr z, Arr vx, Arr vy, Arr vz, Arr h,
                                    Arr c11, Arr c12, Arr c13, Arr c22, Arr c23, Arr c33, Arr mass, Arr rho, Arr p,
                                    Arr c, Arr wh, Arr whd, double n) {
        Fixture f(x.size());
        SoaStd ld{ptr(x),   ptr(y),   ptr(z),   ptr(vx),   ptr(vy),  ptr(vz), ptr(h), ptr(c11), ptr(c12),
                  ptr(c13), ptr(c22), ptr(c23), ptr(c33), ptr(mass), ptr(rho), ptr(p), ptr(c)};
        HT ax, ay, az, maxvs;
        double du;
        momentumEnergyStdJLoop(0, K, openBox(lo, hi), f.nbr.data(), 1, f.nc, ld, kernel(wh, whd, n), ax, ay, az, du,
                               maxvs);
        return py::make_tuple(ax, ay, az, du, maxvs);
    });

    // ------------------------------------------------------------------ all targets, CSR lists, general box and kernel
    m.def("xmass_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y, Arr z,
                          Arr h, Arr mass, Arr wh, Arr whd, double n, int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &h, &mass});
        Csr nl(off, idx, N);
        Box box = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        SoaPos ld{ptr(x), ptr(y), ptr(z), ptr(mass), nullptr};
        auto xm = out1(N);
        for (size_t i = 0; i < N; ++i)
            xm.mutable_data()[i] = xmassJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ptr(h)[i], ld, kf);
        return xm;
    });

    m.def("ve_def_gradh_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y,
                                 Arr z, Arr h, Arr mass, Arr xm, Arr wh, Arr whd, double n, int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &h, &mass, &xm});
        Csr nl(off, idx, N);
        Box box = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        SoaPos ld{ptr(x), ptr(y), ptr(z), ptr(mass), ptr(xm)};
        auto kx = out1(N), gradh = out1(N);
        for (size_t i = 0; i < N; ++i)
            veDefGradhJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ptr(h)[i], ld, kf, kx.mutable_data()[i],
                            gradh.mutable_data()[i]);
        return py::make_tuple(kx, gradh);
    });

    // volumes numer/denom: xm/kx (VE) or m/rho (STD)
    m.def("iad_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y, Arr z,
                        Arr h, Arr numer, Arr denom, Arr wh, Arr whd, double n, int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &h, &numer, &denom});
        Csr nl(off, idx, N);
        Box box = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        SoaIad ld{ptr(x), ptr(y), ptr(z), ptr(numer), ptr(denom), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        auto c = out6(N);
        for (size_t i = 0; i < N; ++i)
        {
            HT ci[6];
            iadJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ptr(h)[i], ld, kf, ci);
            for (int k = 0; k < 6; ++k)
                c.mutable_data()[size_t(k) * N + i] = ci[k];
        }
        return c;
    });

    m.def("divv_curlv_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y,
                               Arr z, Arr vx, Arr vy, Arr vz, Arr h, Arr c6, Arr kx, Arr xm, Arr wh, Arr whd, double n,
                               int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &vx, &vy, &vz, &h, &kx, &xm});
        Csr nl(off, idx, N);
        Rows6 c(c6, N);
        Box box = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        SoaIad ld{ptr(x), ptr(y), ptr(z), nullptr, nullptr, ptr(vx), ptr(vy), ptr(vz), ptr(xm), nullptr, nullptr};
        auto divv = out1(N), curlv = out1(N);
        auto dV = out6(N);
        for (size_t i = 0; i < N; ++i)
        {
            HT ci[6], g[6];
            for (int k = 0; k < 6; ++k)
                ci[k] = c.r[k][i];
            divvCurlvJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ptr(h)[i], ptr(kx)[i], ci, ld, kf,
                           divv.mutable_data()[i], curlv.mutable_data()[i], g);
            for (int k = 0; k < 6; ++k)
                dV.mutable_data()[size_t(k) * N + i] = g[k];
        }
        return py::make_tuple(divv, curlv, dV);
    });

    m.def("av_switches_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y,
                                Arr z, Arr vx, Arr vy, Arr vz, Arr h, Arr c, Arr c6, Arr kx, Arr xm, Arr divv, Arr wh,
                                Arr whd, double n, int choice, double dt, double alphamin, double alphamax, double decay,
                                Arr alpha) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &vx, &vy, &vz, &h, &c, &kx, &xm, &divv, &alpha});
        Csr nl(off, idx, N);
        Rows6 cc(c6, N);
        Box box = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        SoaIad ld{ptr(x), ptr(y), ptr(z), ptr(xm), ptr(kx), ptr(vx), ptr(vy), ptr(vz), nullptr, ptr(c), ptr(divv)};
        auto out = out1(N);
        for (size_t i = 0; i < N; ++i)
        {
            HT ci[6];
            for (int k = 0; k < 6; ++k)
                ci[k] = cc.r[k][i];
            out.mutable_data()[i] = avSwitchesJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ptr(h)[i], ci, ld,
                                                    kf, dt, alphamin, alphamax, decay, ptr(alpha)[i]);
        }
        return out;
    });

    m.def("momentum_energy_all", [](bool avClean, double K, double Atmin, double Atmax, Vec3 lo, Vec3 hi,
                                    std::vector<int> bc, OffArr off, IdxArr idx, Arr x, Arr y, Arr z, Arr vx, Arr vy,
                                    Arr vz, Arr h, Arr c6, Arr mass, Arr c, Arr xm, Arr kx, Arr prho, Arr alpha, Arr dV6,
                                    Arr wh, Arr whd, double n, int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &vx, &vy, &vz, &h, &mass, &c, &xm, &kx, &prho, &alpha});
        Csr nl(off, idx, N);
        Rows6 cc(c6, N), dv(dV6, N);
        SphConsts sc{};
        sc.K     = K;
        sc.Atmin = float(Atmin);
        sc.Atmax = float(Atmax);
        sc.ramp  = float(1.0 / (Atmax - Atmin));
        SoaMom ld{ptr(x),  ptr(y),  ptr(z),  ptr(vx), ptr(vy),   ptr(vz), ptr(h),  cc.r[0],   cc.r[1],   cc.r[2],
                  cc.r[3], cc.r[4], cc.r[5], ptr(mass), ptr(c), ptr(xm), ptr(kx), ptr(prho), ptr(alpha)};
        SoaGradV ldg{{dv.r[0], dv.r[1], dv.r[2], dv.r[3], dv.r[4], dv.r[5]}};
        Box box     = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        auto ax = out1(N), ay = out1(N), az = out1(N), du = out1(N), vs = out1(N);
        for (size_t i = 0; i < N; ++i)
        {
            HT a[3], mv;
            double dui;
            if (avClean)
                momentumEnergyJLoop<true>(unsigned(i), sc, box, nl.list(i), 1, nl.count(i), ld, ldg, kf, a[0], a[1], a[2],
                                          dui, mv);
            else
                momentumEnergyJLoop<false>(unsigned(i), sc, box, nl.list(i), 1, nl.count(i), ld, ldg, kf, a[0], a[1],
                                           a[2], dui, mv);
            ax.mutable_data()[i] = a[0];
            ay.mutable_data()[i] = a[1];
            az.mutable_data()[i] = a[2];
            du.mutable_data()[i] = dui;
            vs.mutable_data()[i] = mv;
        }
        return py::make_tuple(ax, ay, az, du, vs);
    });

    m.def("momentum_energy_std_all", [](double K, Vec3 lo, Vec3 hi, std::vector<int> bc, OffArr off, IdxArr idx, Arr x,
                                        Arr y, Arr z, Arr vx, Arr vy, Arr vz, Arr h, Arr c6, Arr mass, Arr rho, Arr p,
                                        Arr c, Arr wh, Arr whd, double n, int choice) {
        const size_t N = x.size();
        sameSize(N, {&y, &z, &vx, &vy, &vz, &h, &mass, &rho, &p, &c});
        Csr nl(off, idx, N);
        Rows6 cc(c6, N);
        SoaStd ld{ptr(x),  ptr(y),  ptr(z),  ptr(vx),  ptr(vy),   ptr(vz),  ptr(h), cc.r[0], cc.r[1],
                  cc.r[2], cc.r[3], cc.r[4], cc.r[5], ptr(mass), ptr(rho), ptr(p), ptr(c)};
        Box box     = boxOf(lo, hi, bc);
        KernelFn kf = kernel(wh, whd, n, choice);
        auto ax = out1(N), ay = out1(N), az = out1(N), du = out1(N), vs = out1(N);
        for (size_t i = 0; i < N; ++i)
        {
            HT a[3], mv;
            double dui;
            momentumEnergyStdJLoop(unsigned(i), K, box, nl.list(i), 1, nl.count(i), ld, kf, a[0], a[1], a[2], dui, mv);
            ax.mutable_data()[i] = a[0];
            ay.mutable_data()[i] = a[1];
            az.mutable_data()[i] = a[2];
            du.mutable_data()[i] = dui;
            vs.mutable_data()[i] = mv;
        }
        return py::make_tuple(ax, ay, az, du, vs);
    });
}
