// The one place that maps runtime (model id, joint count, chain, precision, QP mode and flags) to template arguments.
// Every launcher picks its kernel instance through these; adding a joint count or a compiled model
// changes this table (and the model list of tmpc_models.h), not the launchers.
// Host-only and free of HIP headers: tests/host_dispatch_check.cpp builds it with a plain C++ compiler.
//
// Each helper calls f with a tag for the matching candidate.  The candidates are named in ascending order,
// each before the recursion to the next: the compiler emits a file's kernel instances in the order they are
// first named, so this order (and the order of the launch_* functions in a file) fixes the code object's layout.
#pragma once
#include <type_traits>

namespace tmpc {

constexpr int NJMAX = 12;
constexpr int NXMAX = 2 * NJMAX;
// joint counts with every kernel instance (fp32 / mixed, soft and hard limits, iLQR, the HBM-row QP, ...);
// 8..NJMAX joints run the SQP on the runtime model (ModelRef), fp64, without box limits, up to 1024 Schur
// rows: a "wide" model
constexpr int NJ_FULL = 7;
template <int NJ>
constexpr bool kWide = NJ > NJ_FULL;

template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<V>{}) for the V of LO, LO + STEP, ... <= HI equal to v; -2 (no instance) if there is none
template <int LO, int HI, int STEP = 1, class F>
int for_nj(int v, F&& f) {
  if constexpr (LO > HI) {
    return -2;
  } else {
    if (v == LO) {
      f(Int<LO>{});
      return 0;
    }
    return for_nj<LO + STEP, HI, STEP>(v, f);
  }
}

// f(Int<V>{}) for every V of LO, LO + STEP, ... <= HI, in order (the set_max_lds lists)
template <int LO, int HI, int STEP = 1, class F>
void for_each_nj(F&& f) {
  if constexpr (LO <= HI) {
    f(Int<LO>{});
    for_each_nj<LO + STEP, HI, STEP>(f);
  }
}

// what a model dispatch hands its callable: Launch<T::nj, T::chain, typename T::model>
template <int NJ, bool CHAIN, class MT>
struct ModelTag {
  static constexpr int nj = NJ;
  static constexpr bool chain = CHAIN;
  using model = MT;
};

// the compiled models (tmpc_models.h: StaticModels); each has ID (> 0), n and chain
template <class... Ms>
struct ModelList {};

// A non-zero mid equal to a compiled model's ID: that model, with its own n and chain.  Otherwise the
// runtime model RT: 1..NJ_FULL joints as a chain or a general tree, NJ_FULL+1..NJMAX joints on the
// general-topology instance only (a chain is a tree; one instance per joint count keeps the build's size).
template <class RT, class... Ms, class F>
int for_model(ModelList<Ms...>, int mid, int nj, bool chain, F&& f) {
  // (a left fold: the models are tried, and their instances first named, in list order)
  if (mid != 0 && (... || (mid == Ms::ID ? (f(ModelTag<Ms::n, Ms::chain != 0, Ms>{}), true) : false))) return 0;
  return for_nj<1, NJMAX>(nj, [&](auto n) {
    constexpr int NJ = decltype(n)::value;
    if constexpr (kWide<NJ>) {
      f(ModelTag<NJ, false, RT>{});
    } else {
      if (chain) f(ModelTag<NJ, true, RT>{});
      else f(ModelTag<NJ, false, RT>{});
    }
  });
}

// f(float{}) for the fp32 dynamics (tmpc_options.precision F32 / MIXED; instances for up to NJ_FULL
// joints only), f(double{}) otherwise
template <int NJ, class F>
void with_real(bool f32, F&& f) {
  if constexpr (!kWide<NJ>) {
    if (f32) {
      f(float{});
      return;
    }
  }
  f(double{});
}

// The instance tables of the QP kernels (tmpc_qp.hip for_qp, tmpc_hooks.hip for_qp_blocks) walk their template
// axes with the two helpers below.  A launch passes each axis its runtime value and reaches one instance; the
// set_max_lds lists pass EVERY and reach all of them -- one table, so neither can name an instance the other lacks.
constexpr int EVERY = -1;

// f(std::true_type{}) for a set flag v, f(std::false_type{}) for a clear one; EVERY: both, true first.
// HAS_TRUE = false: the axis has no `true` instances (a set flag then reaches nothing)
template <bool HAS_TRUE = true, class F>
void with_bool(int v, F&& f) {
  if constexpr (HAS_TRUE) {
    if (v != 0) f(std::true_type{});
  }
  if (v <= 0) f(std::false_type{});
}

// what a QP launch does (QpArgs::mode): prologue + PCG + epilogue, the Schur blocks only, the epilogue only
enum { QP_MODE_PCG = 0, QP_MODE_SCHUR = 1, QP_MODE_DXU = 2 };

// f(Int<MODE>{}) for the QP_MODE_* equal to mode (none for any other value); EVERY: all three, in order
template <class F>
void with_qp_mode(int mode, F&& f) {
  if (mode == QP_MODE_PCG || mode == EVERY) f(Int<QP_MODE_PCG>{});
  if (mode == QP_MODE_SCHUR || mode == EVERY) f(Int<QP_MODE_SCHUR>{});
  if (mode == QP_MODE_DXU || mode == EVERY) f(Int<QP_MODE_DXU>{});
}

}  // namespace tmpc
