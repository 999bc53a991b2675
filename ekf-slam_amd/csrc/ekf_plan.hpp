// The host planner: turns messages into MsgDesc descriptors and a launch list, and keeps the
// per-filter mirror of what the device will hold once the plan has run (Σ parity, pending predict,
// the last pipelined chunk, odometry). It sets every descriptor flag of the project; k_plan_replay
// (plan_kernels.hip) reproduces known() byte for byte, k_plan_assoc unknown() on a chunk route
// (tests/test_plan_assoc_host.py). Nothing here calls HIP, so it is tested on the CPU alone
// (tests/test_plan_host.py).
#pragma once
#include <array>
#include <cstddef>
#include <vector>

#include "ekf_device.hpp"

namespace ekfslam {

struct Launch {
  LaunchKind kind;
  size_t off;  // first descriptor
  int f0, nf, kw;
  bool nolook;  // some active filter's chunk gathers its own Σ_in (no kLook rebuild)
  bool stage;   // some active filter stages rebuild operands behind this chunk's Σ pass (kStageOut)
};

class Planner {
 public:
  // F filters of N landmarks. resident: Σ stays in registers (no kLook, no Joseph chunks);
  // staging: kLook chains read staged rebuild operands (kStageOut / kStageIn).
  void init(int F, int N, bool resident, bool staging);

  // ---- message input: slot k holds the message of filter f0 + k of the next known / unknown ----
  // One message into slot 0. ids == nullptr: unknown association. Known: DELETE markers dropped,
  // EKF_E_RANGE on an id outside [0, N).
  int set_message(int m, const int* ids, const int* actions, const double* rel_xy);
  // One message per filter (ekf_batch_sensor layout) into slots 0..F−1, odometry included;
  // counts[f] == 0: filter f is absent. Validates everything first: a rejected batch changes nothing.
  int load_batch(int assoc_mode, int m_max, const int* counts, const int* ids, const int* actions,
                 const double* rel_xy, const double* odom);
  const char* absent() const { return absent_.data(); }  // load_batch's, [F]
  int size(int k) const { return static_cast<int>(msgs_[k].size()); }
  int largest(int nf) const;  // max(1, markers of slots 0..nf−1)
  void set_odom(int f, double theta, double x, double y) { odom_[f] = {theta, x, y}; }

  // ---- planning: appends to the plan ----
  // Known association, one message per filter in [f0, f0+nf): predict + chunks of ≤ kMaxChunk
  // corrections + posterior (slam.cpp:180-316). absent[k] (batch paths): filter f0+k receives no
  // message this step — its descriptor is inactive, nothing of it changes (an empty MarkerArray is
  // rejected before anything changes, EKF_E_EMPTY).
  void known(int f0, int nf, bool predict, const char* absent = nullptr);
  // Unknown association (slam.cpp:318-530), markers [i0, i1) of each filter's message. route
  // (EKF_ASSOC_*): whole chunks of ≤ kMaxChunk through k_assoc_msg, or (EKF_ASSOC_MARKER) per
  // marker the association kernel + a single-marker launch pair. Decisions land in
  // FilterCtl::assoc_j/new at slot i % kMaxAssoc.
  void unknown(int f0, int nf, bool predict, bool posterior, int i0, int i1, const char* absent,
               int route);
  void posterior(int f);

  // ---- state changes ----
  // The filter's next chunk has no planned predecessor (upload, association, posterior, reset,
  // device plan, host write of its state): it gathers its own Σ_in, nothing is staged for it.
  void forget(int f);
  void reset(int f);  // a fresh filter: parity 0, nothing pending, forget
  void set_pending(int f, bool on) { pending_[f] = on ? 1 : 0; }
  // A simple-form chain cannot rebuild from a Joseph chunk's record (its V columns): the first
  // chunk of each filter after a switch gathers its rows from Σ instead (no kLook). The caller has
  // flushed: what is planned runs with the form it was planned in.
  void set_joseph(bool on);
  void export_state(PlanState* st) const;  // [F]: the mirror, for a device planner
  void adopt(const PlanState* st);         // [F]: ... and back
  // A device-written plan ran: parity_after[F], odom_after[F][3], no pending predict, forget
  void take(const int* parity_after, const double* odom_after);
  // The plan went to the device. The resident kernel keeps no chunk record between launches.
  void clear();

  // ---- queries ----
  const std::vector<Launch>& launches() const { return plan_l_; }
  const std::vector<MsgDesc>& desc() const { return plan_d_; }
  bool joseph() const { return joseph_; }
  int parity(int f) const { return parity_[f]; }
  bool pending(int f) const { return pending_[f] != 0; }
  const std::array<double, 3>& odom(int f) const { return odom_[f]; }  // t_odom_robot (θ, x, y)
  int prev_m(int f) const { return prev_m_[f]; }
  const std::array<int, kMaxChunk>& prev_ids(int f) const { return prev_ids_[f]; }

 private:
  struct Marker {
    int id;
    double zr, zb;
  };
  struct Staged {  // a pipelined chunk of the plan: its descriptor and its launch (−1: none)
    long desc = -1, launch = -1;
  };
  MsgDesc* fill(size_t at, int m, int flags, int f);

  int F_ = 0, N_ = 0;
  bool resident_ = false, staging_ = false, joseph_ = false;
  // mirror
  std::vector<std::array<double, 3>> odom_;  // t_odom_robot (θ, x, y), MsgDesc::odom's order
  std::vector<int> parity_;
  std::vector<char> pending_;
  std::vector<int> prev_m_;  // ≥ 0: last chunk was a pipelined pair (its record is valid)
  std::vector<std::array<int, kMaxChunk>> prev_ids_;  // that chunk's landmark ids
  std::vector<std::array<Staged, 2>> staged_;  // its last two pipelined chunks in this plan ([0]
                                               // the last): kStageOut planning
  // launch plan: descriptors for a whole call (or a whole replay) uploaded with ONE copy
  std::vector<MsgDesc> plan_d_;
  std::vector<Launch> plan_l_;
  // scratch
  std::vector<std::vector<Marker>> msgs_;
  std::vector<char> absent_;  // batch paths: counts[f] == 0, the filter gets no message this step
};

}  // namespace ekfslam
