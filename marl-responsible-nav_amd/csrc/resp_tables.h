// resp_tables.h — the two 10 x 10 f64 tables of custom/Responsibility.py, computed on the host at
// gw_create so that no kernel divides:
//     out[vm * 10 + va]       Resp = clip((vm - va) / (vm + EPS), -1, 1)   (:194-198)
//     out[100 + vm * 10 + va] FeAL = clip(va / (vm + EPS), -1, 1)         (:282-285)
// evaluated in IEEE f64 exactly as numpy does (vm, va = valid-move counts 0..9, EPS = 1e-6).
// Host only and free of HIP, so that a stand-alone program can print it (tools/feal_table_check.cpp).
#ifndef RESP_TABLES_H
#define RESP_TABLES_H

namespace gwtab {

inline double clip1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

// volatile: one rounded IEEE operation each, whatever the host compiler's contraction / precision
inline void fill(double (&out)[200]) {
    for (int vm = 0; vm < 10; ++vm)
        for (int va = 0; va < 10; ++va) {
            volatile double num = (double)vm - (double)va;
            volatile double den = (double)vm + 0.000001;
            const double r = num / den;
            out[vm * 10 + va] = clip1(r);
            volatile double fnum = (double)va;
            const double f = fnum / den;
            out[100 + vm * 10 + va] = clip1(f);
        }
}

// Resp(v, v) is exactly +0.0 for v = 0..9: fear_full_kernel (gw_set_fear_full) relies on it for the row
// of an actor that plays its MdR
inline bool resp_diag_zero(const double (&tab)[200]) {
    for (int v = 0; v < 10; ++v)
        if (tab[v * 10 + v] != 0.0 || 1.0 / tab[v * 10 + v] < 0.0) return false;
    return true;
}

}  // namespace gwtab
#endif  // RESP_TABLES_H
