// hk_arena.h -- one arena per lane, register-resident (v3 of the step kernel).
//
// Reference mapping (hockey/hockey_env.py; Box2D 2.3 for world.Step, restated by the CPU test oracle):
//   presolve()        HockeyEnv.step pre-solve half :659-680 (translation :436-470, boundaries :420-434,
//                     rotation :472-483, puck damping :610-616, hold :618-620, shoot :622-633)
//   world_step()      world.Step(0.02, 180, 60) :682 = Collide -> Solve -> SolveTOI -> ClearForces
//   begin_contact()   ContactDetector.BeginContact :44-76
//   observe*/info*    _get_obs :485-498, obs_agent_two :500-516, _get_info :542-566,
//                     get_info_agent_two :568-591, rewards :518-540
//   basic_opponent()  BasicOpponent.act :787-833
//
//
// The per-arena code by phase:
//   hk_body.h     the register body file: Dyn, Arena, the LDS layout, pick / place, the b2Body accessors and setters
//   hk_collide.h  Collide: far tests, interior rectangles, begin_contact, narrow_phase, pair_update*, collide
//   hk_world.h    Solve and SolveTOI on hk_solver.h: solve_islands, toi_*, solve_toi, world_step
//   hk_game.h     the step laws, observations, info, reward and basic_opponent
#pragma once
#include "hk_body.h"
#include "hk_collide.h"
#include "hk_world.h"
#include "hk_game.h"

#undef SC
