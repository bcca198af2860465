// For the host harness that pins the three launches per step of a rescaled rollout
// (rollout_env_loop_harness.cpp): a kernel side whose fused policy + env step does not
// rescale the actions itself.  rollout_loop.cpp asks, is told "no" and keeps
// ga_action_rescale_f32 between the policy step and the env step.
extern "C" int ga_policy_env_step_rescales(void) { return 0; }
