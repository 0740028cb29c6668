// Device-only helpers of the in-loop features' kernels (the recorders, nudging, breeding, assimilation): the short vector types and
// loads and stores through pointers that come out of a descriptor table.  Such a pointer is generic to the compiler (flat loads and
// stores); it is a device-memory address, and saying so gives the global forms.  T: a scalar or one of the vector types.
#pragma once
#include <hip/hip_runtime.h>

namespace spd {

typedef double double2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2v; };
template <> struct Pair<float> { using type = float2v; };

template <typename T>
__device__ __forceinline__ T load_global(const T *p) {
    return *(const __attribute__((address_space(1))) T *)p;
}
template <typename T>
__device__ __forceinline__ void store_global(T *p, T v) {
    *(__attribute__((address_space(1))) T *)p = v;
}
// ... with the non-temporal hint: values read once / written once that nothing on the device touches again (stream_store.hpp)
template <typename T>
__device__ __forceinline__ T stream_load_global(const T *p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) T *)p);
}
template <typename T>
__device__ __forceinline__ void stream_store_global(T *p, T v) {
    __builtin_nontemporal_store(v, (__attribute__((address_space(1))) T *)p);
}

// the two elements at p (8- or 16-byte aligned) as one access
template <typename T>
__device__ __forceinline__ typename Pair<T>::type load_pair(const T *p) {
    return load_global(reinterpret_cast<const typename Pair<T>::type *>(p));
}
template <typename T>
__device__ __forceinline__ void store_pair(T *p, typename Pair<T>::type v) {
    store_global(reinterpret_cast<typename Pair<T>::type *>(p), v);
}
template <typename T>
__device__ __forceinline__ typename Pair<T>::type stream_load_pair(const T *p) {
    return stream_load_global(reinterpret_cast<const typename Pair<T>::type *>(p));
}
// a pair as it is stored (float where the model stores its physics arrays as fp32) -> doubles
__device__ __forceinline__ double2v widen(double2v v) { return v; }
__device__ __forceinline__ double2v widen(float2v f) {
    double2v x;
    x.x = static_cast<double>(f.x);
    x.y = static_cast<double>(f.y);
    return x;
}

// a pair of doubles into a ring of T (double, or float rounded to nearest) at element `at`: written once, read by the host's gather only
template <typename T>
__device__ __forceinline__ void ring_store(void *ring, long at, double2v v) {
    typename Pair<T>::type out;
    out.x = static_cast<T>(v.x);
    out.y = static_cast<T>(v.y);
    stream_store_global(reinterpret_cast<typename Pair<T>::type *>(static_cast<T *>(ring) + at), out);
}

__device__ __forceinline__ double2v both(double v) {
    double2v r;
    r.x = v;
    r.y = v;
    return r;
}

}  // namespace spd
