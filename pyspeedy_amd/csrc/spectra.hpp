// Spectra by total wavenumber and global means of the spectral state, recorded by the device loop of a multi-step call or computed
// on the state as it stands (spectra.hip holds the kernels, the configuration and the C ABI: spd_model_spectra_* of
// include/pyspeedy_amd.h; the definition is DESIGN section 4d).
#pragma once
#include <hip/hip_runtime.h>

struct spd_model;

namespace spd {

// The names, in the order of their bits in SpectraArgs::mask.
enum SpectraName {
    SPECTRA_KE_ROT = 0,
    SPECTRA_KE_DIV,
    SPECTRA_T,
    SPECTRA_Q,
    SPECTRA_LNPS,
    SPECTRA_T_MEAN,
    SPECTRA_Q_MEAN,
    SPECTRA_LNPS_MEAN,
    SPECTRA_NNAMES
};
constexpr int kSpectraBins = 32;  // total wavenumbers l = 0 ... 31

// doubles a member holds of a name: [8][32], [32], [8] or [1]
constexpr int spectra_per_member(int name) {
    return name <= SPECTRA_Q ? 8 * kSpectraBins : name == SPECTRA_LNPS ? kSpectraBins : name == SPECTRA_LNPS_MEAN ? 1 : 8;
}

// Passed by value.  The sources are member 0, time level 1 of the model's spectral state; out[name] is where member `out_first`
// of that name goes (a ring slot's member 0 with out_first = 0, or a caller's array whose first entry is member `first`).
struct SpectraArgs {
    const double *vor, *div, *t, *tr;  // [M][2][8][992] complex
    const double *ps;                  // [M][2][992] complex
    const double *elm2;                // (31,32): a^2 / (l (l + 1)) at k = m + 31 n, 0 at l = 0
    double *out[SPECTRA_NNAMES];
    unsigned mask;  // bit `name`: wanted
    int first, out_first;
};

// Unroll the ring of one name into dst[count][nt][per] doubles: sample t of the read lies in slot (slot0 + t) % capacity; src: slot
// 0, member `first` of the name; slot_stride in doubles (M * per).
hipError_t run_spectra_gather(const double *src, double *dst, int per, long slot_stride, int count, int nt, int slot0, int capacity,
                              hipStream_t s);

// The step loop's sample of the members [first, first + count), number n since the last reset, behind the step just issued on `s`.
hipError_t spectra_sample(spd_model *m, int first, int count, long long n, hipStream_t s);

}  // namespace spd
