// The data plan: what a problem is staged as -- basis mode, bins per lane, padding, the
// factorised basis, the geometric-grid ratios and the staged bytes -- decided in one pure host
// function of the problem (plan_data.cpp).  No HIP call and no environment read happens in it:
// the switches are handed in (schedule.h), and fitoct_api.cpp uploads what it returns.
#pragma once
#include <vector>

#include "fitoct.h"
#include "kernel_params.h"
#include "schedule.h"

namespace fitoct {

struct DataPlan {
  int bpt = 0, nnp = 15, ppl = 1;   // bins per gradient lane (0: streamed), the kernel's NNP, PPL
  bool mixed = false;
  // every data field of the launch parameters but the device pointers, which stay NULL here:
  // mode, N, n_pad, Nn, D, family, prior_PD, geo*, theta0, S0inv, the priors' scalars, theta_rate
  KParams kp{};
  std::vector<char> staged;       // cx | y | isu | B at n_pad bins, float (mixed) or double
  // MODE_POLY: K^-1 [Nn][Nn] and b [Nn] (MODE_ROWS: what a refused factorisation left, unused)
  std::vector<double> kinv, bv;
  // the plan's host copies of x | y | uy and of the basis rows [N][Nn] (fitoct_plan::h_xyu, h_B)
  std::vector<double> h_xyu, h_B;
};

// The data plan of one problem.  force_bpt >= 0: a batch's common bin layout (0: streamed);
// poly_only: no resident rows (a batch with a problem of N > 2 GT).  FITOCT_OK, or the status
// with its message in fitoct_last_error().
int plan_data(const fitoct_problem* p, int precision, const Switches& sw, int force_bpt,
              bool poly_only, DataPlan& out);

// The data plans of a batch's problems at the batch's common bin layout (plans[0].bpt): every
// tile runs the widest layout any problem plans to, a problem that planned to fewer bins per
// lane is planned again at it, and where one of them cannot take the 16-bin layout (no
// arithmetic depth grid) all are streamed.  Refuses problems that differ in prior_type or Nn,
// or that plan to different kernels; a problem's own failure is prefixed "problem p: ".
int plan_batch_data(const fitoct_problem* probs, int n_problems, int precision,
                    const Switches& sw, std::vector<DataPlan>& plans);

}  // namespace fitoct
