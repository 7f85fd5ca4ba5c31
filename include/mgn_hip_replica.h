/* Replica groups and the group forms of Adam and of the resident parameters: a part of mgn_hip.h, which includes it between its
 * extern "C" braces behind the mgn_group_* calls (mgn_group, mgn_config and mgn_adam_desc are declared there).  Include mgn_hip.h, not
 * this file.  It is a file of its own because the checks of the handle forms (tests/test_params_dev_host.py,
 * tests/test_step_datapoints_host.py) pin that the symbol list read from mgn_hip.h itself holds no group form of them.           */
#ifndef MGN_HIP_H
#error "include mgn_hip.h: mgn_hip_replica.h is a part of it"
#endif

/* ---- replica groups: a minibatch of datapoints split over devices, Adam in place ---------------------------------------------------
 * Derivative training runs on meshes too small to partition (a processor step is launch-bound), so more devices can only serve it by
 * data parallelism.  mgn_group_create_replicas makes a group whose nreplicas handles each hold the WHOLE mesh: mgn_group_create's
 * workers (worker k selects devices[k] once; ordinals may repeat; MGN_DEVICE_NONE for every k gives a host-only group), every handle
 * made with rank = 0, nranks = 1, device = devices[k] -- an ordinary one-partition handle, so two edge sets and ln_dims = MGN_LN_ALL are
 * legal -- and one MGN_COMM_LOCAL communicator that belongs to the GROUP (the handles have none; it is rebuilt after a failed call).
 * Refusals are mgn_group_create's for the same mistakes: MGN_E_ARG for nreplicas outside 1 .. 64, NULL pointers, a mix of
 * MGN_DEVICE_NONE and devices; whatever mgn_create refuses.
 * Every mgn_group_* call above, on a replica group, is the mgn_* call of the same name on every replica with the caller's arguments:
 * the replicas stay identical copies, replica 0 writes the caller's outputs; mgn_group_latents_checksum returns replica 0's sums.
 * Replicas that share a device ordinal take turns in every call that holds no collective (one-partition handles capture and replay
 * hipGraphs; one thread per device at a time enters them); replicas on different devices run side by side.
 *
 * mgn_group_step_datapoints is mgn_step_datapoints for the group: step! on the B listed datapoints of the resident trajectory, the
 * gradient of their mean loss.  loss and losses ([B] or NULL) are host memory; grads is host memory or NULL (nothing of parameter size
 * leaves the devices: the gradient stays in a buffer the group owns on every rank's device, for mgn_group_adam_update).
 *   Replica group: contiguous chunks in listed order -- with q = B / P, r = B % P replica k takes B_k = q + (k < r) entries from
 *   k q + min(k, r) -- each through the plain mgn_step_datapoint (B_k = 1) or mgn_step_datapoints (B_k > 1) with a device buffer as
 *   grads; a replica with B_k = 0 computes no step but joins what follows.  One allgather on every replica's stream, then one launch
 *   per replica writes  g[i] = (float) sum over k ascending, B_k > 0, of ((double) B_k / (double) B) * (double) g_k[i],  the sum starting
 *   from +0.0, every product and every sum rounded once in double, nothing contracted, no atomics: the same bits on every replica,
 *   bitwise repeatable.  losses[b] is the share call's value; loss = (float)((sum_b (double) losses[b]) / B), taken on the host in
 *   listed order.  accumulate != 0 keeps mgn_step_datapoints' rule (accumulate all B first, in listed order, normalise afterwards):
 *   EVERY replica adds all B datapoints to its own totals, then runs its share without accumulating -- totals, counts, calls and maps
 *   are on every replica the bits one handle holds after mgn_step_datapoints with the same list.  The share calls block for their
 *   losses as they do on a handle; behind them the call has one synchronisation, at its end.
 *   Every check comes before any launch or collective on any replica, and the rule of the call is the rule of its LARGEST share: if
 *   some B_k > 1, what mgn_step_datapoints refuses at B > 1 (two edge sets and MGN_LN_ALL: MGN_E_UNSUPPORTED; B_k N or B_k E beyond
 *   int32: MGN_E_ARG) is refused for the whole call, otherwise mgn_step_datapoint's checks apply.  B < 1, a share above
 *   MGN_DATAPOINT_BATCH_MAX, NULL datapoints / mask / loss, a datapoint outside [0, T - 2], an empty mask, a mask entry out of range,
 *   mask_index_base other than 0 / 1, n_grads != mgn_param_count: MGN_E_ARG; no trajectory, dtype != MGN_F32: MGN_E_STATE; host-only:
 *   MGN_E_HIP.  The group stays usable after each.
 *   Partition group (mgn_group_create): B == 1 is mgn_group_step_datapoint's computation and bits (every rank ends with the complete
 *   gradient, kept in the group's buffer on its device); B > 1 at nranks > 1 is MGN_E_STATE before any collective ("drives one
 *   partition"); nranks == 1 is the plain call.
 * mgn_group_set_params_dev, mgn_group_adam_init, mgn_group_adam_state: the handle calls on every rank, with HOST pointers every rank
 * reads in place (reading state returns rank 0's: all ranks hold the same).  mgn_group_get_params_dev copies rank `rank`'s resident
 * vector to the host (MGN_E_ARG for rank outside [0, P)): how a caller checks that the ranks agree.  mgn_group_adam_update with
 * grads == NULL applies mgn_adam_update on every rank to the gradient the last successful mgn_group_step_datapoints left on that
 * rank's device -- no copy, no host work, no traffic between devices; MGN_E_STATE before the first such call, MGN_E_HIP on a host-only
 * group.  With a host pointer every rank reads that array.  The other refusals are the handle calls', on the first failing rank.
 * A training iteration is two calls, mgn_group_step_datapoints(grads = NULL) and mgn_group_adam_update(NULL), on either kind of group.
 * Not built: replicas across processes (RCCL), replicas of partition groups, overlap of the gather with the backward pass.           */
int mgn_group_create_replicas(const mgn_config* cfg, int32_t nreplicas, const int32_t* devices /* [nreplicas] HIP ordinals; may repeat */,
                              mgn_group** out);
int mgn_group_step_datapoints(mgn_group* g, const int32_t* datapoints, int32_t B, int32_t accumulate, const int32_t* mask, int64_t nmask,
                              int32_t mask_index_base, float* grads /* host, or NULL */, size_t n_grads, float* loss,
                              float* losses /* host [B], or NULL */);
int mgn_group_set_params_dev(mgn_group* g, const float* packed /* host */, size_t n);
int mgn_group_get_params_dev(mgn_group* g, int32_t rank, float* packed /* host */, size_t n);
int mgn_group_adam_init(mgn_group* g, const mgn_adam_desc* a);
int mgn_group_adam_update(mgn_group* g, const float* grads /* host, or NULL */, size_t n_grads);
int mgn_group_adam_state(mgn_group* g, int32_t write, float* mt, float* vt, double beta_t[2]); /* host arrays */
