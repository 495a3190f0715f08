// dz_ode.h -- the stiff solver behind likelihoods.MassActionODELogLike: one lane (or one host loop iteration) integrates one point's
// mass-action network from t0 through every output time with an L-stable, stiffly accurate Rosenbrock pair (Rodas4, Hairer & Wanner,
// "Solving ODEs II", IV.7) and adds each output time's Gaussian residuals as it lands on it.
//
// The network itself comes from generated code (likelihoods._ode_source): a struct with
//     static constexpr int S, R, O;                                    species, reactions, observables (compile-time)
//     static bool rates(const double* x, double* k);                   k[R] from the point; false if one is not finite
//     static void rhs(const double* k, const double* y, double* f);    f = N v(y), straight-line code
//     static void jac(const double* k, const double* y, double* J);    J[S*S] (row-major) = N dv/dy, every entry written
//     static void obs(const double* y, double* o);                     o[O]
// The same translation unit is compiled for gfx950 (hipcc --genco) and for the host (clang++ / g++), both with -ffp-contract=off. The
// code uses only + - * /, explicit fma inside dexp / dlog below, comparisons and integer bit operations: no libm or ocml call, no sqrt
// (the error norm's root is folded into the controller's exponent), so both builds give the same bits for every point.
//
// Data block (doubles), built by the Python class:
//   [0] C = sum over the observed entries of (-log sd - log(2 pi) / 2)    [1] rtol   [2] atol   [3] max_steps   [4] t0   [5] T
//   [6, 6+S) y0,   then t[T],   data[T*O] (time-major),   sd[T*O]   (an unobserved entry: data 0, sd +inf -- it adds exactly 0)
//
// With several experimental conditions (MassActionODELogLike(conditions=...)) the block is a two-double header [0] C  [1] stride followed
// by C sub-blocks of stride doubles, each in the layout above (its own C_c, y0, data and sd; rtol .. T and t the same in all): the work
// item w of the *_item_batch kernels is condition w % C of point w / C and integrates from sub-block w % C; see integrate_conditions.
//
// EVENTS (MassActionODELogLike(events=...)): dosing and wash-out during an experiment.  An event (time, species, factor, amount) sets
// y[species] = factor * y[species] + amount at `time` (two roundings: a product, then a sum).  A network of an object that has at least
// one event in some experiment carries
//     static constexpr int EVENTS = Emax;                              the largest event count over the object's experiments, 1..16
// and each experiment's block (each sub-block, with conditions) grows after sd[T*O] by
//     E_c, this experiment's event count (0..Emax),   then Emax records (time, species, factor, amount), sorted by time, padded with zeros
// so that the conditions' stride stays uniform.  The block of a network without events is what it always was.  The semantics:
//   * integration runs in SEGMENTS between breakpoints: t0, the event times and the output times; a segment's last step is clipped so
//     that it lands exactly on the breakpoint; max_steps counts the attempted steps of a segment;
//   * an output at time tau is taken before the events at tau (measure, then intervene), so an event at t[T-1] has no effect; the events
//     at t0 are part of the start: they are applied to y0 before the start step is computed (and before an output at t0);
//   * events at one time apply in the order given;
//   * after the events at a time tau the controller restarts: h = start_step(y_after, rtol, atol, max(t[T-1] - tau, 1e-300)), the formula
//     used at t0, rejected = false, the segment's step count 0; a start step that is not finite or not > 0 is a failed integration; the
//     count of accepted steps (nsteps_out) keeps running;
//   * a point that is not live applies nothing and takes no step.
// Event times come from the block, so control flow stays uniform within a lane group.  integrate_fixed ignores events.
//
// EQUILIBRATION (MassActionODELogLike(equilibrate=...)): an experiment that starts from the resting state of the unstimulated system, a
// state that depends on the point.  A network of an object that equilibrates in at least one experiment carries
//     static constexpr bool EQUILIBRATE = true;
// and each experiment's block (each sub-block, with conditions) grows at its very end -- after the event records if there are any, else
// after sd -- by six doubles
//     on (0 / 1),   rtol_ss,   atol_ss,   horizon,   max_step,   max_steps_ss
// (an experiment without the phase: six zeros), so the conditions' stride stays uniform.  The block of a network without the member is
// what it always was.  The phase (dzode::equilibrate) runs inside integrate between the shape's init and the first start step:
//   * it starts from the experiment's y0 (a Monomial entry as always);
//   * the system is autonomous, so the phase keeps NO CLOCK: only the state and the step size exist;
//   * the first step is start_step(y0, rtol, atol, horizon); not finite or not > 0: a failed integration.  The steps and the controller
//     are integrate's (error test, negativity rule, rejection rule, step_factor, the experiment's rtol and atol), but no step is clipped
//     to a breakpoint and after an accepted step h = min(h * fac, max_step);
//   * the STEADY-STATE TEST runs before every attempted step, so also on y0 itself: the state is steady when
//         drift2(y) * horizon * horizon <= 1,     drift2(y) = the shape's wnorm2(f(y), y, rtol_ss, atol_ss)
//     -- left alone for the length of the experiment the state would move by less than the tolerance, in the RMS sense;
//   * -inf when the state is not steady after max_steps_ss attempted steps (the test runs once more after the last of them), a state is
//     not finite, the iteration matrix is singular or a step is not > 0;
//   * the state at which the test passed is the experiment's start: from there everything is as without the phase -- the events at t0
//     are applied to it (a stimulus is a bolus (t0, s, 1, dose)), the controller starts with the usual formula from that state, an
//     output at t0 sees the equilibrated state after the events at t0; nsteps_out includes the phase's steps;
//   * a point that is not live takes no step; `on`, the tolerances and the limits come from the block and the test's result is one
//     value per lane group, so control flow stays uniform within a group.
// integrate_fixed ignores the phase, as it ignores events.  With conditions every item equilibrates on its own.
//
// Every loop is bounded: at most max_steps_ss attempted steps of the phase, at most max_steps attempted steps per segment, at most
// T + Emax segments.
//
// MONOMIALS (likelihoods.Monomial): a rate constant, a start amount, an observable's scale factor or the argument of a Gaussian
// constraint may be 10**(c + sum_i e_i x[i]), a product of powers of the sampled constants.  The arithmetic is the same on device and
// host and does not depend on rate_scale:
//     s = c;   for the indices i in ascending order  s = s + e_i * x[i]  (e_i = +1: s = s + x[i], e_i = -1: s = s - x[i]);
//     value = dzode::dexp(s * 2.302585092994046)
// so only + - * and dexp are used and both builds give the same bits.  A point is not live (-inf) if a coordinate that a monomial reads
// is not finite or if a monomial's value is not finite (an underflow to 0 is allowed, as for 10**x).  A network that uses one carries
//     static constexpr bool MONOMIALS = true;
//     static bool live(const double* x);                               every monomial outside the rate constants is finite (those: rates)
//     static double y0_row(int r, const double* x, double b);          species r's start amount: the block's b, or for b = NaN the monomial
//                                                                      (a select over constants: no branch on r)
//     static void scale(const double* x, double* o);                   o[q] = scale_q * o[q], at every output time
//     static double constraints(const double* x);                      (only with constraints) g = G0 + acc, G0 = sum(-log sd_m - log(2 pi) / 2),
//                                                                      acc = 0, then for m ascending acc = acc - 0.5 r r, r = (v_m - loc_m) / sd_m
// and the entry points below pass the point's row x to the shape.  g is added to the value of a single experiment (l + g) and, with
// conditions, to the term of condition 0 (l_0 + g); a network without these members compiles to what it compiled to before they existed.
//
// RATE LAWS (likelihoods.RateLaw, likelihoods.Hill): a reaction's rate may be
//     v = k * prod_s y_s^order_s * prod_m h_m(y)
// with kinetic orders that are the reactants' coefficients or the RateLaw's own, and up to 4 Hill factors of one species each,
//     h = y^n / (K^n + y^n) (activation)   or   h = K^n / (K^n + y^n) (repression),     n = 1..8,
// K a parameter (10**x[i] under "log10": dexp(x[i] * 2.302585092994046); x[i] under "linear"), a fixed number > 0 or a monomial.  dy/dt
// stays N v.  The arithmetic, the same on device and host and in every shape, written once per generator (likelihoods._hill_value,
// _hill_slope, _rate_product, _rate_slope):
//   * SLOTS: every distinct (K, n) pair of the network is evaluated once per point, when its rate constants are, in the order of first
//     use: Kn = K * K * ... * K, n factors multiplied left to right.  Slot m lives behind the rate constants: k[R + m] (the one-lane
//     long form: behind its distinct parameters; the lane group and the wave: entry R + m of the point's LDS row, evaluated by lane
//     (R + m) % L).  A network with at least one carries
//         static constexpr int SLOTS = H;                              and R + H stays within the shape's reaction limit
//         static double slot(int m, const double* x, bool& good);      (the group form; the one-lane rates() fills its slots itself)
//   * LIVENESS: a point is not live (-inf) if a coordinate that a K reads is not finite, a K is not finite, or a Kn is not finite or
//     not > 0.  Under "linear" a sampled K <= 0 rejects the point; nothing divides by zero.
//   * THE FACTOR at y:  yn = y * y * ... * y (n factors, left to right);  den = Kn + yn;  h = yn / den  or  h = Kn / den.
//   * ITS DERIVATIVE:  num = ((n * Kn) * y) * ... * y  (n - 1 factors of y, left to right; n = 1: num = Kn);  h' = num / (den * den),
//     for repression (-num) / (den * den).
//   * THE PRODUCT v is taken left to right: k, the mass-action factors y_s (order_s times each) in ascending species, then the Hill
//     factors in the order given.
//   * THE PRODUCT RULE: dv / dy_q is the sum, in that same order, of the mass-action term (if q has a kinetic order c: the product with
//     c * y_q^(c-1) in y_q^c's place, as for plain mass action) and one term per Hill factor on q (the product with h' in h's place);
//     with more than one term: ((t_0) + (t_1)) + ...  A species may be in `order` and in a factor, or in two factors.
//   * Nothing is clamped: a slightly negative amount (one the negativity rule admits) passes through odd powers with its sign; a den that
//     is 0 or not finite makes a rate that is not finite, a failed integration.
// The Jacobian stays analytic, straight-line code with every entry written.  A network without a RateLaw generates the source it always
// did, and compiles to what it compiled to before the member existed.
//
// NOISE (likelihoods.Noise, MassActionODELogLike(noise=...)): the spread of an observable's measurement as a sampled quantity.  For an
// observable q with a Noise(sigma, rel, dist, scale) the residual's scale is no number of the data block but a function of the point:
//   * PER-POINT VALUES: a_q = sigma_q and b_q = rel_q (0 without rel) are evaluated once per point, when its rate constants are, with
//     the arithmetic of a rate constant (a parameter: dexp(x[i] * 2.302585092994046) under "log10", x[i] under "linear"; a monomial: its
//     sum and one dexp; a fixed number: itself), and never again per output time.  Value 2q of the network is a_q, value 2q + 1 is b_q:
//     the one-lane shape keeps the 2 O of them in registers beside the rate constants; the lane group and the wave keep them in the
//     point's LDS row behind everything else (group_lds_row counts them), value m evaluated by lane m % L.
//   * LIVENESS: a point is not live (-inf) if a coordinate that a Noise reads is not finite, an a_q is not finite or not > 0, or a b_q
//     is not finite or < 0.  Under "linear" a sampled sigma <= 0 rejects the point.
//   * THE ENTRY'S TERM at an output time j, with m = o[q] after scale, and d = data, w = sd from the block (for such an observable sd
//     is a fixed WEIGHT, the replicate's relative precision):
//         scale "lin":   s = a_q   (with rel: s = a_q + b_q * dabs(m));   s = s * w;   r = (m - d) / s
//         scale "log":   the block's data slot holds ln d, computed on the host;   s = a_q * w;   r = (dlog(m) - lnd) / s
//         dist "normal":    acc = acc - 0.5 * r * r;   acc = acc - dlog(s);
//         dist "laplace":   acc = acc - dabs(r);       acc = acc - dlog(s);
//   * AN UNOBSERVED ENTRY has w = +inf in the block, as always, and contributes exactly 0 by a select on w, whatever m is -- also
//     m <= 0 on the log scale.
//   * A FAILED INTEGRATION (-inf): an observed entry at which m is not finite, the scale is "log" and m is not > 0, or s is not
//     finite or not > 0.
//   * THE CONSTANT C (blk[0]) is the sum over the observed entries of: -log sd - log(2 pi) / 2 for an observable without a Noise, as
//     always; -log(2 pi) / 2 for "normal"; -log 2 for "laplace"; on the "log" scale additionally -ln d.  w is inside s and not in C.
//   * Entries are visited in the loop's order, j and then q; an observable without a Noise runs the two statements it always ran; sim
//     holds the scaled observables on the natural scale.
// A network with at least one Noise carries
//     static constexpr bool NOISE = true;
//     static double noise_value(int m, const double* x, bool& good);   value m of the point and its liveness (no Noise: NaN; no rel: 0)
//     static bool noise_terms(const double* nz, const double* o, const double* dat, const double* sd, double& acc);
//                                                                      one output time's O entries, q ascending, straight-line code with q
//                                                                      a constant (nz: the 2 O values; dat, sd: the time's rows of the block);
//                                                                      false: a failed integration
// and a network without one generates the source, and the data block, it always did.
//
// INPUTS (likelihoods.Input, MassActionODELogLike(inputs=...)): a measured or prescribed time course u_i(t), piecewise linear, that drives
// the network as one more species.  Nothing produces or consumes an input species; reactions may read it as a catalyst, a kinetic order
// or the species of a Hill factor.  Its right-hand side is the current segment's slope, its Jacobian row is zero, and its value is set
// exactly at every knot, so the system stays autonomous: Rodas4's coefficients and the clock-free equilibration phase remain correct.
// A network with I = 1..4 inputs carries
//     static constexpr int INPUTS = I;
//     static constexpr int DRIVE = D;                                  entry D + i of the point's values k is input i's DRIVE, entry
//                                                                      D - I + i its GAIN g_i (1 without one); D: behind rates and slots
//     static int input_species(int i);                                 the species input i is carried by (a select, no branch on i)
//     static double input_scaled(int i, const double* k, double v);    g_i * v, one product; v itself for an input without a gain
//     static double gain(int i, const double* x, bool& good);          (the group form; the one-lane rates() fills the gains itself)
// and each experiment's block (each sub-block, with conditions) grows at its very end -- after the equilibration's six doubles, the
// event records, or sd, whichever is last -- by
//     K_c, this experiment's count of working knots (I..Kmax),   then Kmax records (time, input, value, slope), sorted by time and at
//     one time by input, padded with zeros
// so that the conditions' stride stays uniform; Kmax <= 128 over all inputs of an experiment together.  The working knots are made in
// Python, once: for every input one knot at t0 (the table's value there and the slope of the segment that holds t0), then the table's
// knots strictly inside (t0, t[T-1]), each with its value and the slope of the segment that follows.  The block of a network without
// inputs is what it always was.  The semantics, the same in both builds and every shape:
//   * THE GAIN g_i (a parameter under rate_scale, a fixed number or a monomial) is evaluated once per point, when the rate constants
//     are, with a rate constant's arithmetic.  A point is not live (-inf) if a coordinate that a gain reads is not finite, or g_i is not
//     finite or not > 0.
//   * A DUE KNOT (time, i, v, s) sets y[species_i] = g_i * v -- one product; without a gain v itself, so a gain that is exactly 1 gives
//     the bits of no gain -- which removes accumulated rounding, and sets the drive to g_i * s, one product, computed when the knot is
//     applied and not per stage.  The input's right-hand side is exactly that drive.  Inputs at one time apply in ascending index.
//   * KNOTS ARE BREAKPOINTS beside t0, the event times and the output times: a step is clipped to land exactly on a knot.  The
//     controller is NOT restarted there: a clipped step leaves its size alone, exactly as at an output time.  max_steps counts per
//     segment.
//   * AT A TIME tau the order is: an output at tau first (measure, then intervene), then the knots due at tau, then the events due at
//     tau in the order given.  The knots at t0 are part of the start, like the events at t0: applied before the start step and before an
//     output at t0.
//   * THE START: the block's y0 entry of an input species is 0.  Ahead of an equilibration phase every input is HELD at its value at
//     t0 with drive 0 -- the knots at t0 applied with slope 0 --, and the phase runs in that state: the resting state under the basal
//     input.  Then, with or without the phase, the knots at t0 are applied as they are, which installs the first slopes before the
//     events at t0 and the start step.
//   * The drive is per-experiment state, not a rate constant: with conditions on the host the point's rate constants and gains are
//     computed once and every condition starts by holding its inputs.  The one-lane shape keeps the drives in registers beside k; the
//     lane group and the wave keep gains and drives in 2 I more doubles of the point's LDS row (dz_ode_group.h).
//   * Knot times come from the block, so control flow stays uniform within a lane group.  integrate_fixed ignores inputs (every drive
//     0, the input species at the block's 0), as it ignores events.
// Every loop stays bounded: at most T + Emax + Kmax segments.
//
// VIEWS (MassActionODELogLike(conditions=[dict(params={i: target}), ...])): condition-specific parameters.  Condition c does not read
// the point x but its VIEW of it, x'_c = V_c(x), a row of P doubles, P one more than the largest index the network reads: entry i is
// x[j] for a target j (an int) or the number v for a target v (a float; the coordinate's value, not the constant: a bare rate index
// under "log10" then gives 10**v), and x[i] itself where the condition says nothing.  A network of an object in which some condition
// has a non-empty mapping carries
//     static constexpr int VIEW = P;                                   1..128
// and every experiment's block grows at its very end -- behind the input knots, the equilibration's six doubles, the event records, or
// sd, whichever is last -- by 2 P doubles, the pairs (j_i, v_i) for i = 0..P-1: j_i >= 0 selects x[j_i], j_i = -1 selects v_i.  A
// condition without a mapping gets the identity (i, 0), an index nothing reads (-1, 0).  Views exist only with conditions, so the
// table's address is the sub-block's end, blk + stride - 2 P.  The block, the source and the code object of a network without the
// member are what they always were.  The contract, the same in both builds and every shape:
//   * SELECT, NO ARITHMETIC: x'[i] is a select between x[j_i] and v_i (view_entry): the bits are exactly one or the other, and x[j_i]
//     is not read where j_i < 0.  A coordinate of the point that a condition does not read has no effect on that condition's term,
//     whatever it holds, NaN included.  An index mapped away in every condition is FORMAL: it is never read from the point and may lie
//     at or beyond the point's length d; Python validates 0 <= j_i < d, so a table never indexes outside the point's row.
//   * WHAT ITEM c RETURNS: its term l_c(x) has the bits of the object of condition c alone, made without a view, evaluated at the row
//     x'_c -- everything an item evaluates (rate constants, slots, gains, noise values, y0 Monomials, scale) reads x'_c; its simulate
//     slice, steps and resting state likewise.
//   * LIVENESS IS PER ITEM: a non-finite coordinate that condition 1 replaces and condition 0 reads makes l_0 = -inf and leaves l_1
//     finite.  The sum stays ((l_0 + l_1) + l_2) + ...
//   * THE HOST BUILD evaluates the rate constants, slots, gains and noise values per condition (integrate_conditions: integrate_point
//     at x'_c), where without a view it evaluates them once per point.
//   * CONSTRAINTS are statements about the point: Python refuses one whose Monomial reads a coordinate that any condition replaces, so
//     they give the same value under every view; they stay on condition 0's term and are evaluated through condition 0's view.
//   * WHERE x' LIVES: one lane per item: a lane-private array of P doubles filled by a loop unrolled over the compile-time P, every
//     index a constant, handed to the generated code in the point's place; a lane group or a wave per item: P more doubles at the end
//     of the group's LDS row (dz_ode_group.h), lane r gathering i = r, r + L, ..., one block-wide barrier ahead of the rate constants.
//
// STEADY OUTPUT (MassActionODELogLike(t=[..., inf], settle=...)): a measurement of the steady state the experiment ends in -- a dose-response
// point, a binding equilibrium, PEtab's time = inf --, the counterpart of EQUILIBRATION at the other end of the experiment.  The object's
// last output time is +inf; t_last is the last finite output time, or t0 if there is none (T = 1).  A network of such an object carries
//     static constexpr bool SETTLE = true;
// tt[T-1] is +inf, row T-1 of data and sd is the steady-state measurement, and EVERY experiment's block (each sub-block, with conditions)
// grows by the phase's six doubles
//     on (always 1: t is shared by the conditions),   rtol_ss,   atol_ss,   horizon,   max_step,   max_steps_ss
// which sit BEHIND the equilibration's six doubles (if the network has them; else behind the event records if there are any, else behind
// sd) and IN FRONT OF the input knots' count K_c and records and of the view pairs, which stay at the block's very end:
//     header, y0, t, data, sd | E_c, events | equilibration's six | SETTLE's six | K_c, knots | view pairs
// The block, the source and the code object of a network without the member are what they always were.  The contract, the same in both
// builds and every shape:
//   1. AT t_last.  The finite outputs run exactly as without the member, with t_last wherever the solver reads "the end of the
//      experiment" (the start step's span at t0 and after events).  At t_last the order at one time holds: the output at t_last, then
//      the knots that are due, then the events that are due in the order given -- an event at t_last, which has no effect in an object
//      with a finite last output, is "measure, intervene, let it settle".  The inputs are then HELD at their value at t_last with every
//      drive 0, as ahead of an equilibration: Python ends the working knots of such an object with one record (t_last, i, u_i(t_last), 0)
//      per input, in ascending i, behind every other knot (also behind the knots at t0 when t_last = t0), so the knots that are due at
//      t_last do the holding and the solver has no code of its own for it.
//   2. THE PHASE is dzode::equilibrate's loop (its instantiation AT_END, below: one loop in the source) on the SETTLE record:
//      h = start_step(y, rtol, atol, horizon), not finite or not > 0: -inf; the steady-state test drift2(y, rtol_ss, atol_ss) * horizon^2
//      <= 1 before every attempted step, so also on the state as it arrives; the step, the error test, the negativity rule and the
//      rejection rule are the experiment's, with its rtol and atol; no step is clipped; after an accepted step h = min(h * fac,
//      max_step); -inf when the state is not steady after max_steps_ss attempts, a state is not finite, the matrix is singular or a step
//      is not > 0.  No clock, no cursor and no record is carried through the loop; the six doubles are read where they are used.
//      Hence the HAND-OVER IDENTITY: the phase applied to a state y gives the bits of the equilibration phase of a second object that
//      starts from y0 = y with `equilibrate` set to the same five numbers.  nsteps_out includes the phase's accepted steps.
//   3. THE OUTPUT.  At the state where the test passed: observe, then the terms of row T-1 by the statements the finite rows run (the
//      network's noise_terms, or the fixed-sd residual): in integrate the phase stands where the steps to a finite output time stand,
//      and the pass then falls into the same output code.  A failure there is -inf, as at a finite row.
//   4. CONTROL FLOW stays uniform within a lane group and a wave: the record comes from the block and the test's result is one value
//      per group.  Lanes of the one-lane shape leave the phase at different counts.  A point that is not live takes no step but stays
//      with its wave.
// Every loop stays bounded: the phase adds at most max_steps_ss attempted steps.  integrate_fixed ignores the phase, as it ignores events.
// Not supported: more than one steady row, a steady state between two finite outputs, Newton polishing of the state (conservation laws
// make the Jacobian singular).
//
// NORMALISED READOUTS (likelihoods.Normalize, MassActionODELogLike(normalize=...)): a readout without an absolute unit -- a blot as a
// fraction of its own maximum, fold change over a chosen point, a trace rescaled to [0, 1].  With m_j the observable after `scale` at
// output row j of one experiment, the data is compared with m'_j = m_j / g ("max": g = max_j m_j; "ref": g = m at the reference row) or
// m'_j = (m_j - lo) / (hi - lo) ("minmax").  g is known only behind the last row, so the rows feed running sums and the term is formed
// once, at the end: for Gaussian residuals the normalised sum of squares is a quadratic form in 1 / g.  A network with at least one
// normalised observable carries
//     static constexpr int NORMALIZE = n;                              the normalised observables, 1..O; number i is the i-th in ascending q
//     static constexpr int NORM_KNOTS = Kmax;                          the knot records of every experiment's block (0 without inputs)
//     static constexpr int NORM_ACC;                                   the doubles beside acc: 2 sums + 1 value per "max" and "ref",
//                                                                      3 sums + 2 values per "minmax" -- only what a kind needs exists
//     static bool normalized(int q);                                   observable q is normalised (a select over constants)
//     static void norm_init(double* na);
//     static void norm_accumulate(const double* rec, int j, const double* o, const double* dat, const double* sd, double* na);
//     static bool norm_finish(const double* rec, const double* nz, const double* na, double& acc);      false: a failed integration
//     static void norm_apply(const double* na, double* row);           one row of sim: m' in m's place
// straight-line code with q a constant, and each experiment's block (each sub-block, with conditions) grows by one RECORD of seven doubles
// per normalised observable, in ascending q,
//     kind (1 "max", 2 "ref", 3 "minmax"),   the reference row (0 unless "ref"),   D,   E,   W,   n_q,   L_q
// which sit BEHIND the input knots (their count and Kmax records; without inputs behind SETTLE's six doubles or whatever is last) and IN
// FRONT OF a view's pairs, which stay at the block's very end because viewed_row finds them there:
//     header, y0, t, data, sd | E_c, events | equilibration's six | SETTLE's six | K_c, knots | norm records | view pairs
// The block, the source and the code object of a network without the member are what they always were.  The contract, the same in both
// builds and every shape:
//   * INTEGRATION UNTOUCHED: steps, states and the un-normalised m have the bits of the object without `normalize`.  An observable
//     without a Normalize adds its row terms exactly as before (the fixed-sd statements, or its part of noise_terms); noise_terms holds
//     nothing for a normalised observable.
//   * EXTREMA AND REFERENCE, at every row in ascending j, observed or not:  hi = m > hi ? m : hi  from -inf;  lo = m < lo ? m : lo  from
//     +inf;  g_ref = m at the reference row ("max": g = hi).
//   * RUNNING SUMS, at every row:  iw = 1.0 / sd  (an unobserved entry has sd = +inf and data 0, so it adds exactly 0),  p = m * iw,
//     e = d * iw;   A = A + p * p;   B = B + p * e;   and for "minmax"  C = C + p * iw.
//   * HOST-SIDE SUMS: D = sum e * e, E = sum e * iw and W = sum iw * iw are computed in Python over the rows from left to right and come
//     from the record, with n_q, the observed count, and L_q = sum ln sd over the observed entries (for an observable with a Noise sd
//     is the weight w).
//   * THE FINISH, behind the last row and so behind all row terms, in ascending q:
//         "max", "ref":   z = 1.0 / g;   Q = (A * z) * z - 2.0 * (B * z) + D
//         "minmax":       g = hi - lo;   A' = A - 2.0 * (lo * C) + (lo * lo) * W;   B' = B - lo * E;   z = 1.0 / g;   Q likewise from A', B'
//         without a Noise:   acc = acc - 0.5 * Q                       (the block's constant keeps -log sd - log(2 pi) / 2 per observed entry)
//         with Noise(sigma): acc = acc - (0.5 * Q) / (a * a);   acc = acc - n_q * dlog(a);   acc = acc - L_q        (a = a_q, the spread is a w)
//     Nothing is clamped.
//   * FAILURE: a g that is not finite or not > 0 is a failed integration: -inf, and NaN in the item's sim slice.  A trajectory that is
//     identically zero has no normalised form.
//   * SIM: with sim given, a pass behind the finish rewrites the slice's normalised columns row by row: m / g, or (m - lo) / (hi - lo).
//     In a lane group o is replicated over the lanes, every lane carries the same sums, and lane 0, which alone holds sim, reads back
//     what it wrote.
//   * VIEWS AND CONDITIONS: every item normalises on its own; item c's term has the bits of the object of condition c alone.
// Only Noise(sigma) -- normal, "lin", no rel -- may stand on a normalised observable: Python refuses the others, whose residuals are no
// quadratic form.  Not supported: a normaliser shared between conditions, a scale fitted to the data.
//
// The stepping loop (dzode::integrate), the controller's formulas, integrate_fixed and the host build's C functions exist once, here, for
// this one-lane solver, for dz_ode_group.h's lane-group solver and for that solver's host twin: see "the one stepping loop" below.
#pragma once
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define DZO_HD __host__ __device__ __forceinline__
#else
#define DZO_HD inline
#endif
#include <stdint.h>
#include <string.h>

// Between the reactions of a long generated sum (likelihoods._ode_long_source, more than 16 reactions): on the device the partial sum
// passes through an empty asm statement, so the compiler keeps the reactions in the order written and holds one rate at a time, not all
// R of them.  Values and order of operations are unchanged.
#if defined(__HIP_DEVICE_COMPILE__)
#define DZODE_FENCE(v) asm volatile("" : "+v"(v))
#else
#define DZODE_FENCE(v) ((void)0)
#endif

namespace dzode {

// ---------------------------------------------------------------- elementary functions
// The engine's dexp / dlog (dz_device.h) and the oracle's orc_exp / orc_log restated for host and device: the same operation sequence
// (fma is correctly rounded on both sides), without dz_device.h's scalar-register constant tricks, which only change instruction selection.
DZO_HD double bits2d(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
DZO_HD uint64_t d2bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
DZO_HD double dfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
DZO_HD double dfloor(double y)            // |y| < 2^62 (dexp's argument range): exact
{
    const double t = (double)(long long)y;
    return t > y ? t - 1.0 : t;
}

DZO_HD double dexp(double x)
{
    if (x != x) return x;
    if (x > 709.782712893384) return __builtin_huge_val();
    if (x < -745.2) return 0.0;
    const double kf = dfloor(x * 1.4426950408889634 + 0.5);
    double r = dfma(-kf, 6.93147180369123816490e-01, x);
    r = dfma(-kf, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = dfma(p, r, 1.0 / 479001600.0);
    p = dfma(p, r, 1.0 / 39916800.0);
    p = dfma(p, r, 1.0 / 3628800.0);
    p = dfma(p, r, 1.0 / 362880.0);
    p = dfma(p, r, 1.0 / 40320.0);
    p = dfma(p, r, 1.0 / 5040.0);
    p = dfma(p, r, 1.0 / 720.0);
    p = dfma(p, r, 1.0 / 120.0);
    p = dfma(p, r, 1.0 / 24.0);
    p = dfma(p, r, 1.0 / 6.0);
    p = dfma(p, r, 0.5);
    p = dfma(p, r, 1.0);
    p = dfma(p, r, 1.0);
    int k = (int)kf;
    if (k < -1000) { p = p * bits2d((uint64_t)(1023 - 1000) << 52); k += 1000; }
    return p * bits2d((uint64_t)(k + 1023) << 52);
}

DZO_HD double dlog(double x)
{
    if (x != x) return x;
    if (x < 0.0) return __builtin_nan("");
    if (x == 0.0) return -__builtin_huge_val();
    if (x == __builtin_huge_val()) return x;
    int e = 0;
    uint64_t b = d2bits(x);
    if ((b >> 52) == 0) { x = x * 18014398509481984.0; e = -54; b = d2bits(x); }
    e += (int)(b >> 52) - 1023;
    double m = bits2d((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = dfma(p, z, 1.0 / 21.0);
    p = dfma(p, z, 1.0 / 19.0);
    p = dfma(p, z, 1.0 / 17.0);
    p = dfma(p, z, 1.0 / 15.0);
    p = dfma(p, z, 1.0 / 13.0);
    p = dfma(p, z, 1.0 / 11.0);
    p = dfma(p, z, 1.0 / 9.0);
    p = dfma(p, z, 1.0 / 7.0);
    p = dfma(p, z, 1.0 / 5.0);
    p = dfma(p, z, 1.0 / 3.0);
    const double t = 2.0 * s;
    const double lm = dfma(t * z, p, t);
    const double ef = (double)e;
    return dfma(ef, 6.93147180369123816490e-01, dfma(ef, 1.90821492927058770002e-10, lm));
}

DZO_HD bool finite(double x) { return x - x == 0.0; }
DZO_HD double dabs(double x) { return x < 0.0 ? -x : x; }
DZO_HD double dmax(double a, double b) { return a > b ? a : b; }
DZO_HD double dmin(double a, double b) { return a < b ? a : b; }

// ---------------------------------------------------------------- monomials: what a network that has them adds (see the head of the file)
template <class Net, class = void> struct has_monomials { static constexpr bool value = false; };
template <class Net> struct has_monomials<Net, decltype((void)Net::MONOMIALS)> { static constexpr bool value = true; };
template <class Net, class = void> struct has_constraints { static constexpr bool value = false; };
template <class Net> struct has_constraints<Net, decltype((void)&Net::constraints)> { static constexpr bool value = true; };

// ... and events (the head of the file): EVENTS is the bound of the event loop and the record count of every experiment's block
template <class Net, class = void> struct has_events { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_events<Net, decltype((void)Net::EVENTS)> {
    static constexpr bool value = true;
    static constexpr int count = Net::EVENTS;
    static_assert(Net::EVENTS >= 1 && Net::EVENTS <= 16, "1..16 events per experiment");
};

// ... and the equilibration phase (the head of the file): the network of an object that equilibrates in at least one experiment
template <class Net, class = void> struct has_equilibrate { static constexpr bool value = false; };
template <class Net> struct has_equilibrate<Net, decltype((void)Net::EQUILIBRATE)> { static constexpr bool value = Net::EQUILIBRATE; };

// ... and the steady output (the head of the file, STEADY OUTPUT): the network of an object whose last output time is +inf
template <class Net, class = void> struct has_settle { static constexpr bool value = false; };
template <class Net> struct has_settle<Net, decltype((void)Net::SETTLE)> { static constexpr bool value = Net::SETTLE; };

// ... and rate laws (the head of the file): SLOTS is the number of distinct Hill (K, n) pairs, the doubles behind the rate constants
template <class Net, class = void> struct has_slots { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_slots<Net, decltype((void)Net::SLOTS)> {
    static constexpr bool value = true;
    static constexpr int count = Net::SLOTS;
    static_assert(Net::SLOTS >= 1 && Net::R + Net::SLOTS <= 256, "reactions plus slots within the shape's reaction limit");
};
// ... and inputs (the head of the file, INPUTS): I piecewise-linear time courses, each a species of its own; their gains and drives
// are 2 I doubles behind the rate constants and slots
constexpr int MAX_INPUT_KNOTS = 128;
template <class Net, class = void> struct has_inputs { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_inputs<Net, decltype((void)Net::INPUTS)> {
    static constexpr bool value = true;
    static constexpr int count = Net::INPUTS;
    static_assert(Net::INPUTS >= 1 && Net::INPUTS <= 4 && Net::DRIVE >= Net::INPUTS, "1..4 inputs, their gains in front of their drives");
};
// the doubles of a point's rate constants and slots (an array of at least one; with inputs: and their gains and drives)
template <class Net> constexpr int rate_doubles()
{
    if constexpr (has_inputs<Net>::value) return Net::DRIVE + Net::INPUTS;
    else return Net::R + has_slots<Net>::count > 0 ? Net::R + has_slots<Net>::count : 1;
}

// ... and sampled noise (the head of the file, NOISE): 2 O per-point values, a_q and b_q
template <class Net, class = void> struct has_noise { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_noise<Net, decltype((void)Net::NOISE)> { static constexpr bool value = true; static constexpr int count = 2 * Net::O; };
// the doubles of a point's noise values (an array of at least one)
template <class Net> constexpr int noise_doubles() { return has_noise<Net>::count > 0 ? has_noise<Net>::count : 1; }

// ... and views (the head of the file, VIEWS): P viewed coordinates per condition, 2 P doubles at the end of every experiment's block
template <class Net, class = void> struct has_view { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_view<Net, decltype((void)Net::VIEW)> {
    static constexpr bool value = true;
    static constexpr int count = Net::VIEW;
    static_assert(Net::VIEW >= 1 && Net::VIEW <= 128, "1..128 viewed coordinates");
};
// the doubles of an item's viewed row (an array of at least one)
template <class Net> constexpr int view_doubles() { return has_view<Net>::count > 0 ? has_view<Net>::count : 1; }

// ... and normalised readouts (the head of the file, NORMALISED READOUTS): NORMALIZE records of seven doubles in every experiment's
// block, NORM_ACC running sums and values beside acc
template <class Net, class = void> struct has_normalize { static constexpr bool value = false; static constexpr int count = 0; };
template <class Net> struct has_normalize<Net, decltype((void)Net::NORMALIZE)> {
    static constexpr bool value = true;
    static constexpr int count = Net::NORM_ACC;
    static_assert(Net::NORMALIZE >= 1 && Net::NORMALIZE <= Net::O && Net::NORM_KNOTS >= 0 && Net::NORM_KNOTS <= 128, "1..O normalised observables");
};
// the doubles of an experiment's running sums and values (an array of at least one)
template <class Net> constexpr int norm_doubles() { return has_normalize<Net>::count > 0 ? has_normalize<Net>::count : 1; }

// Entry i of a condition's view: a select between x[j_i] and v_i, no arithmetic; x is not read where j_i < 0.
DZO_HD double view_entry(const double* x, const double* tab, int i)
{
    const double j = tab[2 * i], v = tab[2 * i + 1];
    return j >= 0.0 ? x[(int)j] : v;
}

// The row an item reads in the point's place: for a network with a view xv[P], gathered from the table at the end of the item's
// sub-block (blk, of stride doubles); else the point's own row.
template <class Net>
DZO_HD const double* viewed_row(const double* x, const double* blk, long long stride, double* xv)
{
    if constexpr (has_view<Net>::value) {
        const double* tab = blk + stride - 2 * Net::VIEW;
#pragma unroll
        for (int i = 0; i < Net::VIEW; ++i) xv[i] = view_entry(x, tab, i);
        return xv;
    } else {
        return x;
    }
}

// The point's noise values nz[2 O] in the order of the contract; false if one of them says that the point is not live.
template <class Net>
DZO_HD bool noise_point(const double* x, double* nz)
{
    bool good = true;
    if constexpr (has_noise<Net>::value) {
#pragma unroll
        for (int m = 0; m < has_noise<Net>::count; ++m) {
            bool g;
            nz[m] = Net::noise_value(m, x, g);
            good = good && g;
        }
    }
    return good;
}

// The drives of a point's inputs set to 0: the array shapes' knot reads the entries it does not write (a select over the unrolled
// index), so they hold a number before the first knot.
template <class Net>
DZO_HD void clear_drives(double* k)
{
    if constexpr (has_inputs<Net>::value) {
#pragma unroll
        for (int m = 0; m < Net::INPUTS; ++m) k[Net::DRIVE + m] = 0.0;
    }
}

template <class Net>
DZO_HD bool monomials_live(const double* x)
{
    if constexpr (has_monomials<Net>::value) return Net::live(x);
    else return true;
}

template <class Net>
DZO_HD double start_amount(int r, const double* x, double b)        // species r's y0: the data block's entry b, or the network's monomial
{
    if constexpr (has_monomials<Net>::value) return Net::y0_row(r, x, b);
    else return b;
}

template <class Net>
DZO_HD void observe_scaled(const double* x, const double* y, double* o)
{
    Net::obs(y, o);
    if constexpr (has_monomials<Net>::value) Net::scale(x, o);
}

template <class Net>
DZO_HD double add_constraints(double l, const double* x, bool first)    // l + g for a live point's single experiment or condition 0
{
    if constexpr (has_constraints<Net>::value) return first ? l + Net::constraints(x) : l;
    else return l;
}

// ---------------------------------------------------------------- dense LU with partial pivoting, unrolled at compile-time S
// a[S*S] row-major, factored in place; the diagonal holds the pivots' reciprocals.  Rows are exchanged with selects over every
// candidate row, so every array index is a constant after unrolling: the matrix lives in registers.  False if a pivot is zero.
template <int S>
DZO_HD bool lu_factor(double* a, int* piv)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        int p = k;
        double best = dabs(a[k * S + k]);
#pragma unroll
        for (int r = k + 1; r < S; ++r) {
            const double v = dabs(a[r * S + k]);
            if (v > best) { best = v; p = r; }
        }
        piv[k] = p;
#pragma unroll
        for (int r = k + 1; r < S; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int c = 0; c < S; ++c) {
                const double u = a[k * S + c], w = a[r * S + c];
                a[k * S + c] = sw ? w : u;
                a[r * S + c] = sw ? u : w;
            }
        }
        ok = ok && best != 0.0;
        const double inv = 1.0 / a[k * S + k];
        a[k * S + k] = inv;
#pragma unroll
        for (int r = k + 1; r < S; ++r) {
            const double l = a[r * S + k] * inv;
            a[r * S + k] = l;
#pragma unroll
            for (int c = k + 1; c < S; ++c) a[r * S + c] = a[r * S + c] - l * a[k * S + c];
        }
    }
    return ok;
}

template <int S>
DZO_HD void lu_solve(const double* a, const int* piv, double* b)
{
#pragma unroll
    for (int k = 0; k < S; ++k) {
#pragma unroll
        for (int r = k + 1; r < S; ++r) {
            const bool sw = piv[k] == r;
            const double u = b[k], w = b[r];
            b[k] = sw ? w : u;
            b[r] = sw ? u : w;
        }
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {
#pragma unroll
        for (int r = k + 1; r < S; ++r) b[r] = b[r] - a[r * S + k] * b[k];
    }
#pragma unroll
    for (int k = S - 1; k >= 0; --k) {
        double s = b[k];
#pragma unroll
        for (int c = k + 1; c < S; ++c) s = s - a[k * S + c] * b[c];
        b[k] = s * a[k * S + k];
    }
}

// ---------------------------------------------------------------- Rodas4
// Hairer & Wanner's RODAS coefficients (METH = 1), for an autonomous system (mass action: no explicit t, so the d_i terms vanish).
// Stages: W k_i = f(y + sum_j a_ij k_j) + (1/h) sum_j c_ij k_j, W = I / (h gamma) - J.  y5 + k5 is the embedded (order 3) solution,
// y5 + k5 + k6 the order-4 one; both stiffly accurate.  k6 is the error estimate.
struct Rodas4 {
    static constexpr double gamma = 0.25;
    static constexpr double a21 = 1.544, a31 = 0.9466785280815826, a32 = 0.2557011698983284;
    static constexpr double a41 = 3.314825187068521, a42 = 2.896124015972201, a43 = 0.9986419139977817;
    static constexpr double a51 = 1.221224509226641, a52 = 6.019134481288629, a53 = 12.53708332932087, a54 = -0.687886036105895;
    static constexpr double c21 = -5.6688, c31 = -2.430093356833875, c32 = -0.2063599157091915;
    static constexpr double c41 = -0.1073529058151375, c42 = -9.594562251023355, c43 = -20.47028614809616;
    static constexpr double c51 = 7.496443313967647, c52 = -10.24680431464352, c53 = -33.99990352819905, c54 = 11.7089089320616;
    static constexpr double c61 = 8.083246795921522, c62 = -7.981132988064893, c63 = -31.52159432874371, c64 = 16.31930543123136,
                            c65 = -6.058818238834054;
};

// One step of size h from y: ynew (order 4), yemb (order 3; may alias nothing) and err2, the mean over species of
// (k6 / (atol + rtol max(|y|, |ynew|)))^2.  False if the iteration matrix is singular.
template <class Net>
DZO_HD bool rodas4_step(const double* k, const double* y, double h, double rtol, double atol, double* ynew, double* yemb, double& err2)
{
    constexpr int S = Net::S;
    typedef Rodas4 M;
    double w[S * S];
    int piv[S];
    Net::jac(k, y, w);
    const double fac = 1.0 / (h * M::gamma), ih = 1.0 / h;
#pragma unroll
    for (int i = 0; i < S * S; ++i) w[i] = -w[i];
#pragma unroll
    for (int s = 0; s < S; ++s) w[s * S + s] = w[s * S + s] + fac;
    const bool ok = lu_factor<S>(w, piv);
    double k1[S], k2[S], k3[S], k4[S], k5[S], k6[S], u[S];
    Net::rhs(k, y, k1);
    lu_solve<S>(w, piv, k1);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = y[s] + M::a21 * k1[s];
    Net::rhs(k, u, k2);
#pragma unroll
    for (int s = 0; s < S; ++s) k2[s] = k2[s] + (M::c21 * k1[s]) * ih;
    lu_solve<S>(w, piv, k2);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = y[s] + M::a31 * k1[s] + M::a32 * k2[s];
    Net::rhs(k, u, k3);
#pragma unroll
    for (int s = 0; s < S; ++s) k3[s] = k3[s] + (M::c31 * k1[s] + M::c32 * k2[s]) * ih;
    lu_solve<S>(w, piv, k3);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = y[s] + M::a41 * k1[s] + M::a42 * k2[s] + M::a43 * k3[s];
    Net::rhs(k, u, k4);
#pragma unroll
    for (int s = 0; s < S; ++s) k4[s] = k4[s] + (M::c41 * k1[s] + M::c42 * k2[s] + M::c43 * k3[s]) * ih;
    lu_solve<S>(w, piv, k4);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = y[s] + M::a51 * k1[s] + M::a52 * k2[s] + M::a53 * k3[s] + M::a54 * k4[s];
    Net::rhs(k, u, k5);
#pragma unroll
    for (int s = 0; s < S; ++s) k5[s] = k5[s] + (M::c51 * k1[s] + M::c52 * k2[s] + M::c53 * k3[s] + M::c54 * k4[s]) * ih;
    lu_solve<S>(w, piv, k5);
#pragma unroll
    for (int s = 0; s < S; ++s) u[s] = u[s] + k5[s];
    Net::rhs(k, u, k6);
#pragma unroll
    for (int s = 0; s < S; ++s) k6[s] = k6[s] + (M::c61 * k1[s] + M::c62 * k2[s] + M::c63 * k3[s] + M::c64 * k4[s] + M::c65 * k5[s]) * ih;
    lu_solve<S>(w, piv, k6);
    double e2 = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        yemb[s] = u[s];
        ynew[s] = u[s] + k6[s];
        const double sk = atol + rtol * dmax(dabs(y[s]), dabs(ynew[s]));
        const double q = k6[s] / sk;
        e2 = e2 + q * q;
    }
    err2 = e2 * (1.0 / S);
    return ok;
}

template <int S>
DZO_HD double wnorm2(const double* v, const double* y, double rtol, double atol)      // mean of (v / (atol + rtol |y|))^2
{
    double e2 = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double q = v[s] / (atol + rtol * dabs(y[s]));
        e2 = e2 + q * q;
    }
    return e2 * (1.0 / S);
}

// ---------------------------------------------------------------- the controller's formulas, shared by every shape
// the step controller: the factor from the error, before the negativity and rejection caps
// err = sqrt(err2); h_new = h * clamp(0.9 err^(-1/4), 0.2, 6), no growth right after a rejection
DZO_HD double step_factor(double err2)
{
    const double fac = err2 > 0.0 ? 0.9 * dexp(-0.125 * dlog(err2)) : 6.0;
    return dmin(6.0, dmax(0.2, fac));
}

// Hairer, Norsett & Wanner I, II.4 starting step, with the norms' roots folded into dexp / dlog; at most span.
DZO_HD double start_h0(double d0, double d1, double span)
{
    return (d0 < 1e-10 || d1 < 1e-10) ? 1e-6 : dmin(0.01 * dexp(0.5 * (dlog(d0) - dlog(d1))), span);
}

DZO_HD double start_h(double h0, double d1, double d2h, double span)      // d2h: the norm of f1 - f0, still to be divided by h0^2
{
    const double m = dmax(d1, d2h / (h0 * h0));                            // max(d1, d2)^2
    const double h1 = m <= 1e-30 ? dmax(1e-6, h0 * 1e-3) : dexp((dlog(0.01) - 0.5 * dlog(m)) * 0.2);
    return dmin(dmin(100.0 * h0, h1), span);
}

// ---------------------------------------------------------------- the one stepping loop
// The log-likelihood of one point (and, with sim != nullptr, the observables at every output time, [T][O]; with nsteps_out, the steps
// that passed the finiteness test).  -inf when the point is not live (a rate constant that is not finite, a point past the batch's end),
// the state is not finite, the iteration matrix is singular, a step underflows or an output interval needs more than max_steps steps.
// Who holds the state is the SHAPE's business.  A shape sh supplies
//     Shape::S, Shape::O, Shape::State                 (S doubles, or one double per lane of a group)
//     sh.init(blk, y)                                  y0 from the data block
//     sh.start_step(y, rtol, atol, span)               the starting step
//     sh.step(y, h, rtol, atol, yn, err2)              one Rodas4 step: the order-4 solution and err2; false if W is singular
//     sh.all_finite(yn, seed)                          seed && every amount of yn finite
//     sh.any_negative(yn, y, rtol, atol)               an amount of yn below -(atol + rtol |y|)
//     sh.observe(y, o)                                 o[O]
//     Shape::EVENTS, sh.apply(y, species, factor, amount)   (a network with events: Emax, and y[species] = factor * y[species] + amount)
//     Shape::EQUILIBRATE, Shape::SETTLE, sh.drift2(y, rtol, atol)   (a network that equilibrates or has a steady output -- either member
//                                                      alone asks for it --: the steady-state test's wnorm2(f(y), y, rtol, atol))
//     Shape::Net, sh.noise()                           (a network with sampled noise: where the point's 2 O noise values are)
//     Shape::INPUTS, sh.knot(y, i, value, slope)       (a network with inputs: I, and y[species_i] = g_i * value, drive_i = g_i * slope)
// and there are three: Array<OneLane<Net>> (below: one lane or one host loop iteration per point), Array<HostGroup<Net, L>> and
// Group<Net, L> (dz_ode_group.h: a group of L lanes per point, and its host twin).  A point that is not live keeps h = 0, ok = false and
// takes no step, but does not return ahead of the loop: the lanes of a group stay with their wave.
// With events (the head of the file) every pass of the outer loop is one SEGMENT: the events that are due and the controller's (re)start
// -- the start at t0 is the first of them, so the start step exists once in the code --, the steps up to the next breakpoint, and the
// output if the breakpoint is one.  A network with inputs (the head of the file, INPUTS) runs in segments too, whether or not it has
// events: the knots at t0 are applied ahead of the loop -- and, without events, the start step computed there as it always was: a
// start step inside the loop is a second copy of the right-hand side in it; with it, and with the records' address and count carried
// through the loop, enzyme13 + input @ 16 took 268 registers and, past 256, ran with half its waves: 1.9 times the time --, and a pass first applies the knots that are due, which does not restart the controller.  Without events
// and inputs a pass is an output interval, as it always was.
// The equilibration phase (the head of the file) of one experiment: y from the experiment's start amounts to the resting state, by the
// steps and the controller of integrate without a clock and without an end time.  ok in: the point is live; out: the state is steady
// (or the experiment does not equilibrate).  nsteps grows by the accepted steps; attempts (optional): the attempted ones.  The loop is
// bounded by the block's max_steps_ss; `on`, the tolerances and the limits come from the block and the test's result is one value per
// lane group, so control flow stays uniform within a group.
// The knot count of one experiment's block (blk: the experiment's block); behind it the records (time, input, value, slope).
template <class Shape>
DZO_HD const double* input_knots(const double* blk)
{
    const long long per = (long long)(int)blk[5] * Shape::O;
    return blk + 6 + Shape::S + (int)blk[5] + 2 * per + (Shape::EVENTS > 0 ? 1 + 4 * Shape::EVENTS : 0) + (Shape::EQUILIBRATE ? 6 : 0) +
           (Shape::SETTLE ? 6 : 0);
}

// The start of an experiment of a network with inputs: every input held at its value at t0 with drive 0 (the knots at t0 with slope 0).
template <class Shape>
DZO_HD void hold_inputs(const Shape& sh, const double* blk, typename Shape::State& y)
{
    if constexpr (Shape::INPUTS > 0) {
        const double* inp = input_knots<Shape>(blk);
        const int K = (int)dmin(inp[0], (double)MAX_INPUT_KNOTS);
#pragma unroll 1
        for (int kn = 0; kn < K && inp[1 + 4 * kn] <= blk[4]; ++kn) sh.knot(y, (int)inp[2 + 4 * kn], inp[3 + 4 * kn], 0.0);
    }
}

// The knots from the cursor kn on that are due at time t, applied in the block's order; the new cursor.  (The records' address and
// the count are formed from the block where they are needed and not carried through the step loop: registers.)
template <class Shape>
DZO_HD int due_knots(const Shape& sh, const double* blk, typename Shape::State& y, int kn, double t)
{
    const double* inp = input_knots<Shape>(blk);
    const int K = (int)dmin(inp[0], (double)MAX_INPUT_KNOTS);
#pragma unroll 1
    for (; kn < K && inp[1 + 4 * kn] <= t; ++kn) sh.knot(y, (int)inp[2 + 4 * kn], inp[3 + 4 * kn], inp[4 + 4 * kn]);
    return kn;
}

// The time of the knot at the cursor, +inf past the last.
template <class Shape>
DZO_HD double next_knot(const double* blk, int kn)
{
    const double* inp = input_knots<Shape>(blk);
    return kn < (int)dmin(inp[0], (double)MAX_INPUT_KNOTS) ? inp[1 + 4 * kn] : __builtin_huge_val();
}

// The records of an experiment's normalised observables (the head of the file, NORMALISED READOUTS): behind the knots' count and Kmax
// records of a network with inputs -- Kmax is the network's NORM_KNOTS --, else where those would begin.  Formed where it is used.
template <class Shape>
DZO_HD const double* norm_records(const double* blk)
{
    return input_knots<Shape>(blk) + (Shape::INPUTS > 0 ? 1 + 4 * Shape::Net::NORM_KNOTS : 0);
}

// (AT_END: the same loop on the steady output's record, which sits behind the equilibration's, from the state at t_last -- the head of
// the file, STEADY OUTPUT; dzode::settle below.  One loop in the source, an instantiation per phase.)
template <class Shape, bool AT_END = false>
DZO_HD bool equilibrate(const Shape& sh, const double* blk, typename Shape::State& y, bool ok, int& nsteps, int* attempts)
{
    const long long per = (long long)(int)blk[5] * Shape::O;
    const double* eq = blk + 6 + Shape::S + (int)blk[5] + 2 * per + (Shape::EVENTS > 0 ? 1 + 4 * Shape::EVENTS : 0) +
                       (AT_END && Shape::EQUILIBRATE ? 6 : 0);
    if (attempts) *attempts = 0;
    if (eq[0] == 0.0) return ok;
    const double rtol = blk[1], atol = blk[2], rtol_ss = eq[1], atol_ss = eq[2], horizon = eq[3], max_step = eq[4];
    const int max_steps = (int)eq[5];
    typename Shape::State yn;
    double h = ok ? sh.start_step(y, rtol, atol, horizon) : 0.0;
    ok = ok && finite(h) && h > 0.0;
    bool rejected = false;
    for (int n = 0; ok; ++n) {
        if (sh.drift2(y, rtol_ss, atol_ss) * horizon * horizon <= 1.0) break;      // steady: before every attempted step, y0 included
        if (n >= max_steps || !(h > 0.0)) { ok = false; break; }
        if (attempts) *attempts = n + 1;
        // from here integrate's step, error test, negativity and rejection rules, repeated and not shared: with one function called from
        // both loops the code objects of networks WITHOUT the phase came out different from what they were (two to three VGPRs more)
        double err2;
        const bool nonsing = sh.step(y, h, rtol, atol, yn, err2);
        if (!sh.all_finite(yn, nonsing && finite(err2))) { ok = false; break; }
        ++nsteps;
        double fac = step_factor(err2);
        const bool neg = sh.any_negative(yn, y, rtol, atol);
        if (neg) fac = dmin(fac, 0.25);
        if (err2 <= 1.0 && !neg) {
            if (rejected) fac = dmin(fac, 1.0);
            y = yn;
            h = dmin(h * fac, max_step);
            rejected = false;
        } else {
            h = h * fac;
            rejected = true;
        }
    }
    return ok;
}

// The steady output's phase (the head of the file, STEADY OUTPUT): equilibrate's loop on the record behind the equilibration's.
template <class Shape>
DZO_HD bool settle(const Shape& sh, const double* blk, typename Shape::State& y, bool ok, int& nsteps, int* attempts)
{
    return equilibrate<Shape, true>(sh, blk, y, ok, nsteps, attempts);
}

// The end of the experiment as the start steps' span reads it: the last output time, or for a network with a steady output t_last, the
// last finite one (t0 if there is none).  Read where it is used and not carried through the loop.  (Only a network with a steady
// output calls it: the others keep the statements they always had, and so their code objects.)
DZO_HD double last_finite_time(const double* tt, int T, double t0) { return T > 1 ? tt[T - 2] : t0; }

// settled (optional; array shapes): the state at which the steady output's test passed; settle_attempts: the phase's attempted steps.
template <class Shape>
DZO_HD double integrate(const Shape& sh, const double* blk, bool live, double* sim, int* nsteps_out,
                        typename Shape::State* settled = nullptr, int* settle_attempts = nullptr)
{
    constexpr int S = Shape::S, O = Shape::O;
    const double rtol = blk[1], atol = blk[2], t0 = blk[4];
    const int max_steps = (int)blk[3], T = (int)blk[5];
    const double* tt = blk + 6 + S;
    const double* dat = tt + T;
    const double* sd = dat + (long long)T * O;
    typename Shape::State y, yn;
    double o[O];
    sh.init(blk, y);
    if constexpr (Shape::EQUILIBRATE) hold_inputs(sh, blk, y);              // (a network with inputs: the phase sees them held at u(t0), every drive 0)
    double t = t0, acc = 0.0;
    constexpr int EV = Shape::EVENTS, IN = Shape::INPUTS;
    constexpr bool SEG = EV > 0 || IN > 0;                                   // the loop's passes are segments between breakpoints
    constexpr bool NORM = has_normalize<typename Shape::Net>::value;          // some observable is normalised to its own time course
    [[maybe_unused]] double na[norm_doubles<typename Shape::Net>()];         // its running sums and values
    if constexpr (NORM) Shape::Net::norm_init(na);
    double h = 0.0;
    bool ok = live, rejected = false;
    int nsteps = 0;
    if constexpr (Shape::EQUILIBRATE) ok = equilibrate(sh, blk, y, ok, nsteps, nullptr);      // y: the resting state, the experiment's start
    [[maybe_unused]] int kn = 0;                                             // the knot cursor
    if constexpr (IN > 0) kn = due_knots(sh, blk, y, kn, t0);               // the knots at t0 are part of the start: the first slopes
    if constexpr (EV == 0) {
        if constexpr (Shape::SETTLE) {
            if (T > 1) {                                                     // (a steady output alone: no finite stretch, no start step for one)
                h = ok ? sh.start_step(y, rtol, atol, dmax(last_finite_time(tt, T, t0) - t0, 1e-300)) : 0.0;
                ok = ok && finite(h) && h > 0.0;
            }
        } else {
            h = ok ? sh.start_step(y, rtol, atol, dmax(tt[T - 1] - t0, 1e-300)) : 0.0;
            ok = ok && finite(h) && h > 0.0;
        }
    }
    // (without events the block ends with sd: evt is then the pointer one past its end, only formed and never read)
    [[maybe_unused]] const double* evt = sd + (long long)T * O + (EV > 0 ? 1 : 0);      // records of (time, species, factor, amount)
    [[maybe_unused]] int ev = 0, E = 0;                                      // the event cursor, this experiment's event count
    [[maybe_unused]] bool fresh = true;                                      // the controller is to be (re)started: at t0, after events
    if constexpr (EV > 0) E = (int)dmin(evt[-1], (double)EV);
    for (int j = 0; ok && j < T;) {
        const double tout = tt[j];
        double tend = tout;                                                  // the segment's end
        if constexpr (IN > 0) kn = due_knots(sh, blk, y, kn, t);             // the knots that are due: the value exactly, the next slope
        if constexpr (EV > 0) {
#pragma unroll 1
            for (; ev < E && evt[4 * ev] <= t; ++ev) {                       // the events that are due, in the order given
                sh.apply(y, (int)evt[4 * ev + 1], evt[4 * ev + 2], evt[4 * ev + 3]);
                fresh = true;
            }
            if constexpr (Shape::SETTLE) {
                if (j == T - 1) fresh = false;                               // (the steady output's pass: the phase has a start step of its own)
            }
            if (fresh) {
                if constexpr (Shape::SETTLE) h = sh.start_step(y, rtol, atol, dmax(last_finite_time(tt, T, t0) - t, 1e-300));
                else h = sh.start_step(y, rtol, atol, dmax(tt[T - 1] - t, 1e-300));
                rejected = false;
                fresh = false;
                if (!(finite(h) && h > 0.0)) { ok = false; break; }
            }
            if (ev < E && evt[4 * ev] < tout) tend = evt[4 * ev];            // (an event at tout: after the output, in the next pass)
        }
        if constexpr (IN > 0) tend = dmin(tend, next_knot<Shape>(blk, kn));  // (a knot at tout: after the output; the controller is not restarted)
        if constexpr (Shape::SETTLE) {
            if (j == T - 1) {                                                // the steady output's pass (tout = +inf): everything due at t_last is applied, the inputs are held
                ok = settle(sh, blk, y, ok, nsteps, settle_attempts);
                if (ok && settled) *settled = y;
                // INVARIANT: nothing is due after t_last -- Python refuses an event beyond it and cuts the working knots there --, so
                // tend is +inf here.  It is set all the same: with a record left over, `tend < tout` below would send the pass round
                // again and the phase would run twice.
                tend = tout;
                t = tout;                                                    // (the clock is not read again)
            }
        }
        for (int n = 0; t < tend; ++n) {
            const bool clip = t + h >= tend;
            const double hs = clip ? tend - t : h;
            if (n >= max_steps || t + hs == t) { ok = false; break; }
            double err2;
            const bool nonsing = sh.step(y, hs, rtol, atol, yn, err2);
            if (!sh.all_finite(yn, nonsing && finite(err2))) { ok = false; break; }
            ++nsteps;
            double fac = step_factor(err2);
            // amounts are non-negative: a step that takes one below -(atol + rtol |y|) is rejected like a failed error test (CVODE's
            // inequality constraints).  Left in, such an undershoot of a species with a second-order loss grows without bound.
            const bool neg = sh.any_negative(yn, y, rtol, atol);
            if (neg) fac = dmin(fac, 0.25);
            if (err2 <= 1.0 && !neg) {
                if (rejected) fac = dmin(fac, 1.0);
                y = yn;
                t = clip ? tend : t + hs;
                h = clip ? dmax(h, hs * fac) : hs * fac;       // (a step clipped to the breakpoint leaves the controller's size alone)
                rejected = false;
            } else {
                h = hs * fac;
                rejected = true;
            }
        }
        if (!ok) break;
        if constexpr (SEG) {
            if (tend < tout) continue;                                       // landed on an event or a knot, not on the output time
        }
        sh.observe(y, o);
        if constexpr (NORM)                                                  // (the head of the file, NORMALISED READOUTS: extrema and sums, every row)
            Shape::Net::norm_accumulate(norm_records<Shape>(blk), j, o, dat + (long long)j * O, sd + (long long)j * O, na);
        if constexpr (has_noise<typename Shape::Net>::value) {               // (the head of the file, NOISE: the network's own terms)
            const bool fine = Shape::Net::noise_terms(sh.noise(), o, dat + (long long)j * O, sd + (long long)j * O, acc);
#pragma unroll
            for (int q = 0; q < O; ++q)
                if (sim) sim[(long long)j * O + q] = o[q];
            if (!fine) { ok = false; break; }
        } else if constexpr (NORM) {                                         // (the statements below for the observables that are not normalised)
#pragma unroll
            for (int q = 0; q < O; ++q) {
                if (!Shape::Net::normalized(q)) {
                    const double r = (o[q] - dat[(long long)j * O + q]) / sd[(long long)j * O + q];
                    acc = acc - 0.5 * r * r;
                }
                if (sim) sim[(long long)j * O + q] = o[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < O; ++q) {
                const double r = (o[q] - dat[(long long)j * O + q]) / sd[(long long)j * O + q];
                acc = acc - 0.5 * r * r;
                if (sim) sim[(long long)j * O + q] = o[q];
            }
        }
        ++j;
    }
    if constexpr (NORM) {                                                    // (the head of the file, NORMALISED READOUTS: the finish, behind all row terms)
        if (ok) {
            if constexpr (has_noise<typename Shape::Net>::value) ok = Shape::Net::norm_finish(norm_records<Shape>(blk), sh.noise(), na, acc);
            else ok = Shape::Net::norm_finish(norm_records<Shape>(blk), nullptr, na, acc);
        }
        if (ok && sim) {                                                     // (the lane that wrote the slice reads it back: m' in m's place)
            for (int j = 0; j < T; ++j) Shape::Net::norm_apply(na, sim + (long long)j * O);
        }
    }
    if (nsteps_out) *nsteps_out = nsteps;
    return ok ? blk[0] + acc : -__builtin_huge_val();
}

// ---------------------------------------------------------------- the array shapes: the whole state in one place
// An algebra ALG says how a step is computed on S doubles: ALG::Net, rates(x, k), rhs(k, y, f), wnorm2(v, y, rtol, atol) and
// step(k, y, h, rtol, atol, ynew, yemb, err2).  OneLane is dz_ode.h's own (row-oriented LU, left-to-right norm), compiled for host and
// device; HostGroup (dz_ode_group.h) mirrors the lane group's operation order.
template <class NET>
struct OneLane {
    typedef NET Net;
    static constexpr int S = Net::S;
    DZO_HD static bool rates(const double* x, double* k) { return Net::rates(x, k) && monomials_live<Net>(x); }
    DZO_HD static void rhs(const double* k, const double* y, double* f) { Net::rhs(k, y, f); }
    DZO_HD static double wnorm2(const double* v, const double* y, double rtol, double atol) { return dzode::wnorm2<S>(v, y, rtol, atol); }
    DZO_HD static bool step(const double* k, const double* y, double h, double rtol, double atol, double* ynew, double* yemb, double& err2)
    {
        return rodas4_step<Net>(k, y, h, rtol, atol, ynew, yemb, err2);
    }
};

template <class Alg>
DZO_HD double start_step(const double* k, const double* y, double rtol, double atol, double span)
{
    constexpr int S = Alg::Net::S;
    double f0[S], y1[S], f1[S];
    Alg::rhs(k, y, f0);
    const double d0 = Alg::wnorm2(y, y, rtol, atol), d1 = Alg::wnorm2(f0, y, rtol, atol);
    const double h0 = start_h0(d0, d1, span);
#pragma unroll
    for (int s = 0; s < S; ++s) y1[s] = y[s] + h0 * f0[s];
    Alg::rhs(k, y1, f1);
#pragma unroll
    for (int s = 0; s < S; ++s) f1[s] = f1[s] - f0[s];
    return start_h(h0, d1, Alg::wnorm2(f1, y, rtol, atol), span);
}

template <class Alg>
struct Array {
    static constexpr int S = Alg::Net::S, O = Alg::Net::O, EVENTS = has_events<typename Alg::Net>::count;
    static constexpr int INPUTS = has_inputs<typename Alg::Net>::count;
    static constexpr bool EQUILIBRATE = has_equilibrate<typename Alg::Net>::value, SETTLE = has_settle<typename Alg::Net>::value;
    typedef typename Alg::Net Net;
    struct State { double v[S]; };
    const double* k;                                   // the rate constants
    const double* x;                                   // the point's row (read only by a network with monomials)
    const double* nz = nullptr;                        // the point's noise values (read only by a network with sampled noise)
    DZO_HD const double* noise() const { return nz; }
    DZO_HD void init(const double* blk, State& y) const
    {
#pragma unroll
        for (int s = 0; s < S; ++s) y.v[s] = start_amount<typename Alg::Net>(s, x, blk[6 + s]);
    }
    DZO_HD double start_step(const State& y, double rtol, double atol, double span) const { return dzode::start_step<Alg>(k, y.v, rtol, atol, span); }
    DZO_HD double drift2(const State& y, double rtol, double atol) const      // the steady-state test's norm of f(y)
    {
        double f[S];
        Alg::rhs(k, y.v, f);
        return Alg::wnorm2(f, y.v, rtol, atol);
    }
    DZO_HD bool step(const State& y, double h, double rtol, double atol, State& yn, double& err2) const
    {
        double ye[S];
        return Alg::step(k, y.v, h, rtol, atol, yn.v, ye, err2);
    }
    DZO_HD bool all_finite(const State& yn, bool fin) const
    {
#pragma unroll
        for (int s = 0; s < S; ++s) fin = fin && finite(yn.v[s]);
        return fin;
    }
    DZO_HD bool any_negative(const State& yn, const State& y, double rtol, double atol) const
    {
        bool neg = false;
#pragma unroll
        for (int s = 0; s < S; ++s) neg = neg || yn.v[s] < -(atol + rtol * dabs(y.v[s]));
        return neg;
    }
    DZO_HD void observe(const State& y, double* o) const { observe_scaled<typename Alg::Net>(x, y.v, o); }
    DZO_HD void apply(State& y, int species, double factor, double amount) const      // (a select over the unrolled s: y stays in registers)
    {
#pragma unroll
        for (int s = 0; s < S; ++s) y.v[s] = s == species ? factor * y.v[s] + amount : y.v[s];
    }
    // A knot of input i: the value into its species, the slope into its drive -- entry DRIVE + i of the caller's own array k, which is
    // per-experiment state and not constant (selects over the unrolled s and m: y and k stay in registers)
    DZO_HD void knot(State& y, int i, double value, double slope) const
    {
        if constexpr (INPUTS > 0) {
            double* drive = const_cast<double*>(k) + Net::DRIVE;
            const int species = Net::input_species(i);
            const double gv = Net::input_scaled(i, k, value), gs = Net::input_scaled(i, k, slope);
#pragma unroll
            for (int s = 0; s < S; ++s) y.v[s] = s == species ? gv : y.v[s];
#pragma unroll
            for (int m = 0; m < INPUTS; ++m) drive[m] = m == i ? gs : drive[m];
        }
    }
};

// One point through an array shape.  The rate constants are tested here, ahead of the loop, and the loop runs with live a constant.
// first: the single experiment, or condition 0 of several -- the term that a network's constraints are added to.
template <class Alg>
DZO_HD double integrate_point(const double* x, const double* blk, double* sim, int* nsteps_out, bool first = true,
                              typename Array<Alg>::State* settled = nullptr, int* settle_attempts = nullptr)
{
    double k[rate_doubles<typename Alg::Net>()];
    [[maybe_unused]] double nz[noise_doubles<typename Alg::Net>()];
    if (nsteps_out) *nsteps_out = 0;
    if (!Alg::rates(x, k)) return -__builtin_huge_val();
    clear_drives<typename Alg::Net>(k);
    if constexpr (has_noise<typename Alg::Net>::value) {
        if (!noise_point<typename Alg::Net>(x, nz)) return -__builtin_huge_val();
        return add_constraints<typename Alg::Net>(integrate(Array<Alg>{k, x, nz}, blk, true, sim, nsteps_out, settled, settle_attempts), x, first);
    } else {
        return add_constraints<typename Alg::Net>(integrate(Array<Alg>{k, x}, blk, true, sim, nsteps_out, settled, settle_attempts), x, first);
    }
}

// The host build's resting state of one point's experiment (blk: one experiment's block): the state handed to the experiment, before
// the events at t0 -- the start amounts themselves where the experiment does not equilibrate, NaN where the point is not live or the
// phase fails.  attempts: the phase's attempted steps.
template <class Alg>
DZO_HD void equilibrate_point(const double* x, const double* blk, double* yss, int* attempts)
{
    constexpr int S = Alg::Net::S;
    double k[rate_doubles<typename Alg::Net>()];
    const Array<Alg> sh{k, x};
    typename Array<Alg>::State y;
    bool ok = Alg::rates(x, k);
    clear_drives<typename Alg::Net>(k);
    *attempts = 0;
    if (ok) {
        sh.init(blk, y);
        hold_inputs(sh, blk, y);
        if constexpr (Array<Alg>::EQUILIBRATE) {
            int steps = 0;
            ok = equilibrate(sh, blk, y, ok, steps, attempts);
        }
    }
    for (int s = 0; s < S; ++s) yss[s] = ok ? y.v[s] : __builtin_nan("");
}

// The host build's settled state of one point's experiment (blk: one experiment's block; the head of the file, STEADY OUTPUT): the state
// at which the steady output's test passed, NaN where the item failed -- the point is not live, the experiment or the phase failed, or
// row T-1's terms did -- and throughout for a network without a steady output.  attempts: the phase's attempted steps.
template <class Alg>
DZO_HD void settle_point(const double* x, const double* blk, double* yss, int* attempts)
{
    constexpr int S = Alg::Net::S;
    typename Array<Alg>::State y;
    *attempts = 0;
    const double v = integrate_point<Alg>(x, blk, nullptr, nullptr, false, &y, attempts);      // (no constraints: the item's own term)
    const bool ok = Array<Alg>::SETTLE && v != -__builtin_huge_val() && v == v;
    for (int s = 0; s < S; ++s) yss[s] = ok ? y.v[s] : __builtin_nan("");
}

// The constraints' term g of one point alone (0 for a network without constraints, -inf for a point that is not live).
template <class Alg>
DZO_HD double constraint_term(const double* x)
{
    double k[rate_doubles<typename Alg::Net>()];
    return Alg::rates(x, k) ? add_constraints<typename Alg::Net>(0.0, x, true) : -__builtin_huge_val();
}

// The host build's noise values of one point alone, ab[O][2] = (a_q, b_q) whether or not the point is live (a network without sampled
// noise: NaN throughout).
template <class Net>
DZO_HD void noise_values(const double* x, double* ab)
{
    if constexpr (has_noise<Net>::value) noise_point<Net>(x, ab);
    else
        for (int m = 0; m < 2 * Net::O; ++m) ab[m] = __builtin_nan("");
}

// The host build's point under C conditions (the data block with the [C, stride] header): the rate constants once, then condition by
// condition in ascending order through the same integrate as a device item, the terms added as k_sum_items adds the items:
// ((l_0 + l_1) + l_2) + ... (l_0 with the constraints' g, if the network has any).  terms[C] (optional): the l_c; sim (optional): [C][T][O]; nsteps_out: the steps of all conditions.
template <class Alg>
DZO_HD double integrate_conditions(const double* x, const double* hdr, double* terms, double* sim, int* nsteps_out)
{
    const int C = (int)hdr[0];
    const long long stride = (long long)hdr[1], per = (long long)(int)hdr[2 + 5] * Alg::Net::O;
    if constexpr (has_view<typename Alg::Net>::value) {      // (the head of the file, VIEWS: everything per condition, at its own row)
        double xv[view_doubles<typename Alg::Net>()], total = 0.0;
        int steps = 0;
        for (int c = 0; c < C; ++c) {
            const double* blk = hdr + 2 + c * stride;
            int st = 0;
            const double v = integrate_point<Alg>(viewed_row<typename Alg::Net>(x, blk, stride, xv), blk, sim ? sim + c * per : nullptr, &st, c == 0);
            if (terms) terms[c] = v;
            total = c == 0 ? v : total + v;
            steps += st;
        }
        if (nsteps_out) *nsteps_out = steps;
        return total;
    }
    double k[rate_doubles<typename Alg::Net>()];
    double nz[noise_doubles<typename Alg::Net>()];
    const bool rated = Alg::rates(x, k);
    clear_drives<typename Alg::Net>(k);
    const bool live = noise_point<typename Alg::Net>(x, nz) && rated;
    double total = 0.0;
    int steps = 0;
    for (int c = 0; c < C; ++c) {
        int st = 0;
        double v = live ? integrate(Array<Alg>{k, x, nz}, hdr + 2 + c * stride, true, sim ? sim + c * per : nullptr, &st) : -__builtin_huge_val();
        if (live) v = add_constraints<typename Alg::Net>(v, x, c == 0);
        if (terms) terms[c] = v;
        total = c == 0 ? v : total + v;
        steps += st;
    }
    if (nsteps_out) *nsteps_out = steps;
    return total;
}

// Fixed steps (the order test only): nsteps steps of (t1 - t0) / nsteps from y0, propagating the order-4 solution (which = 0) or the
// embedded order-3 one (which = 1).  The final state in y; false if a step failed.
template <class Alg>
DZO_HD bool integrate_fixed(const double* x, const double* blk, double t1, int nsteps, int which, double* y)
{
    constexpr int S = Alg::Net::S;
    double k[rate_doubles<typename Alg::Net>()], yn[S], ye[S];
    if (!Alg::rates(x, k)) return false;
    clear_drives<typename Alg::Net>(k);                                      // (inputs are ignored: every drive 0)
#pragma unroll
    for (int s = 0; s < S; ++s) y[s] = start_amount<typename Alg::Net>(s, x, blk[6 + s]);
    const double h = (t1 - blk[4]) / nsteps;
    bool ok = true;
    for (int n = 0; n < nsteps; ++n) {
        double err2;
        ok = Alg::step(k, y, h, blk[1], blk[2], yn, ye, err2) && ok;
#pragma unroll
        for (int s = 0; s < S; ++s) y[s] = which ? ye[s] : yn[s];
    }
    return ok;
}

}  // namespace dzode

// The host build's C functions around an algebra ALG (a plain type name), for the one-lane and the lane-group source alike: those that do
// not depend on the data block's form (dzode_fixed takes one experiment's block), ...
#define DZODE_HOST_COMMON(ALG)                                                                                                          \
    extern "C" int dzode_fixed(const double* x, const double* blk, double t1, int nsteps, int which, double* y)                         \
    {                                                                                                                                    \
        return dzode::integrate_fixed<ALG>(x, blk, t1, nsteps, which, y) ? 1 : 0;                                                       \
    }                                                                                                                                    \
    extern "C" void dzode_constraints(const double* X, long long n, int ld, double* g)                                                  \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i) g[i] = dzode::constraint_term<ALG>(X + i * ld);                                                \
    }                                                                                                                                    \
    extern "C" void dzode_noise(const double* X, long long n, int ld, double* ab)                                                       \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i) dzode::noise_values<ALG::Net>(X + i * ld, ab + i * 2 * ALG::Net::O);                           \
    }                                                                                                                                    \
    extern "C" double dzode_exp(double x) { return dzode::dexp(x); }                                                                     \
    extern "C" double dzode_log(double x) { return dzode::dlog(x); }

// ... those of one experiment ...
#define DZODE_HOST_ENTRIES(ALG)                                                                                                         \
    extern "C" void dzode_loglike(const double* X, long long n, int ld, const double* blk, double* like, int* nsteps)                  \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i) like[i] = dzode::integrate_point<ALG>(X + i * ld, blk, nullptr, nsteps ? nsteps + i : nullptr); \
    }                                                                                                                                    \
    extern "C" void dzode_simulate(const double* X, long long n, int ld, const double* blk, double* sim, double* like)                 \
    {                                                                                                                                    \
        const long long per = (long long)(int)blk[5] * ALG::Net::O;                                                                      \
        for (long long i = 0; i < n; ++i) like[i] = dzode::integrate_point<ALG>(X + i * ld, blk, sim + i * per, nullptr);               \
    }                                                                                                                                    \
    extern "C" void dzode_equilibrate(const double* X, long long n, int ld, const double* blk, double* yss, int* attempts)              \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i) dzode::equilibrate_point<ALG>(X + i * ld, blk, yss + i * ALG::Net::S, attempts + i);          \
    }                                                                                                                                    \
    extern "C" void dzode_settle(const double* X, long long n, int ld, const double* blk, double* yss, int* attempts)                   \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i) dzode::settle_point<ALG>(X + i * ld, blk, yss + i * ALG::Net::S, attempts + i);               \
    }                                                                                                                                    \
    DZODE_HOST_COMMON(ALG)

// ... and those of C conditions (blk: the block with the [C, stride] header): dzode_loglike gives the points' sums (nsteps: over the
// conditions), dzode_simulate the terms [n][C] and, with sim, the observables [n][C][T][O].
#define DZODE_HOST_ITEM_ENTRIES(ALG)                                                                                                    \
    extern "C" void dzode_loglike(const double* X, long long n, int ld, const double* blk, double* like, int* nsteps)                  \
    {                                                                                                                                    \
        for (long long i = 0; i < n; ++i)                                                                                                \
            like[i] = dzode::integrate_conditions<ALG>(X + i * ld, blk, nullptr, nullptr, nsteps ? nsteps + i : nullptr);               \
    }                                                                                                                                    \
    extern "C" void dzode_simulate(const double* X, long long n, int ld, const double* blk, double* sim, double* terms)                \
    {                                                                                                                                    \
        const long long C = (long long)blk[0], per = C * (int)blk[2 + 5] * ALG::Net::O;                                                  \
        for (long long i = 0; i < n; ++i) dzode::integrate_conditions<ALG>(X + i * ld, blk, terms + i * C, sim ? sim + i * per : nullptr, nullptr); \
    }                                                                                                                                    \
    extern "C" void dzode_equilibrate(const double* X, long long n, int ld, const double* blk, double* yss, int* attempts)              \
    {                                                                                                                                    \
        const long long C = (long long)blk[0], stride = (long long)blk[1];                                                               \
        double xv[dzode::view_doubles<ALG::Net>()];                                                                                      \
        for (long long w = 0; w < n * C; ++w) {                                                                                          \
            const double* sub = blk + 2 + (w % C) * stride;                                                                              \
            dzode::equilibrate_point<ALG>(dzode::viewed_row<ALG::Net>(X + (w / C) * ld, sub, stride, xv), sub, yss + w * ALG::Net::S,    \
                                          attempts + w);                                                                                 \
        }                                                                                                                                \
    }                                                                                                                                    \
    extern "C" void dzode_settle(const double* X, long long n, int ld, const double* blk, double* yss, int* attempts)                   \
    {                                                                                                                                    \
        const long long C = (long long)blk[0], stride = (long long)blk[1];                                                               \
        double xv[dzode::view_doubles<ALG::Net>()];                                                                                      \
        for (long long w = 0; w < n * C; ++w) {                                                                                          \
            const double* sub = blk + 2 + (w % C) * stride;                                                                              \
            dzode::settle_point<ALG>(dzode::viewed_row<ALG::Net>(X + (w / C) * ld, sub, stride, xv), sub, yss + w * ALG::Net::S,         \
                                     attempts + w);                                                                                      \
        }                                                                                                                                \
    }                                                                                                                                    \
    DZODE_HOST_COMMON(ALG)

// The entry points around a generated network struct NET: the batch kernel the engine's multi-kernel path launches (one thread per
// point, 256 threads per block: dz_set_likelihood_module with lanes_per_point 1) and the host build's C functions.
#if defined(__HIP__) && !defined(DZODE_PREDICT)
#define DZODE_ENTRIES(NET)                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_batch(const double* X, long long n, int d, int ld, double* like,           \
                                                                  const void* data)                                                    \
    {                                                                                                                                    \
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;                                                            \
        if (i >= n) return;                                                                                                              \
        like[i] = dzode::integrate_point<dzode::OneLane<NET>>(X + i * ld, (const double*)data, nullptr, nullptr);                       \
    }
// ... with C conditions: the same launch over n = points x C ITEMS (dz_set_likelihood_items), one thread per item; item w is condition
// w % C of point w / C -- the condition is the fastest index, so neighbouring lanes integrate the same rate constants from different
// starts -- reads that point's row and writes like[w]; the engine adds a point's C items in ascending order.  The sub-block's address
// differs by lane, so what the one-experiment kernel keeps in scalar registers (rtol, atol, T, the addresses of t, data and sd) is in
// vector registers here; the address passes through DZODE_FENCE so that the compiler carries it as one pointer and not as a base and
// offsets beside it (8 species, 15 reactions, 5 conditions: 12 bytes of scratch without the fence, none with it).
#define DZODE_ITEM_ENTRIES(NET)                                                                                                         \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_item_batch(const double* X, long long n, int d, int ld, double* like,      \
                                                                       const void* data)                                               \
    {                                                                                                                                    \
        const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;                                                            \
        if (w >= n) return;                                                                                                              \
        const double* hdr = (const double*)data;                                                                                         \
        const long long C = (long long)hdr[0], stride = (long long)hdr[1], i = w / C;                                                    \
        const double* blk = hdr + 2 + (w - i * C) * stride;                                                                              \
        DZODE_FENCE(blk);          /* (one opaque pointer per lane: see below) */                                                        \
        double xv[dzode::view_doubles<NET>()];     /* (a network with a view: the item's own row, every index a constant) */            \
        const double* x = dzode::viewed_row<NET>(X + i * ld, blk, stride, xv);                                                           \
        like[w] = dzode::integrate_point<dzode::OneLane<NET>>(x, blk, nullptr, nullptr, w == i * C);                                     \
    }
#elif defined(__HIP__)
// PREDICTION (MassActionODELogLike.device().simulate): the same generated source behind a leading `#define DZODE_PREDICT 1` is a
// translation unit of its own whose entry macros make the PREDICTION kernels instead (dz_set_output_module / dz_eval_outputs): the launch,
// the item arithmetic and the integration of the kernels above -- the same integrate on the same shape from the same block -- with sim
// given: item w's T * O scaled observables go to out[w * out_ld + j * O + q], what the host build's dzode_simulate writes, and its
// term to like[w].  An item whose term is -inf leaves NaN in its whole slice (integrate breaks off in the middle of a failed run: the
// lane that wrote the slice overwrites all of it, entries never reached included; nothing relies on the buffer having been cleared).
namespace dzode {
__device__ __forceinline__ void predict_finish(double term, const double* blk, int O, double* sim)
{
    if (term == -__builtin_huge_val()) {
        const long long per = (long long)(int)blk[5] * O;
        for (long long m = 0; m < per; ++m) sim[m] = __builtin_nan("");
    }
}
}  // namespace dzode
#define DZODE_ENTRIES(NET)                                                                                                              \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_predict(const double* X, long long n, int d, int ld, double* like,         \
                                                                    const void* data, double* out, long long out_ld)                   \
    {                                                                                                                                    \
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;                                                            \
        if (i >= n) return;                                                                                                              \
        const double v = dzode::integrate_point<dzode::OneLane<NET>>(X + i * ld, (const double*)data, out + i * out_ld, nullptr);       \
        like[i] = v;                                                                                                                     \
        dzode::predict_finish(v, (const double*)data, NET::O, out + i * out_ld);                                                         \
    }
#define DZODE_ITEM_ENTRIES(NET)                                                                                                         \
    extern "C" __global__ __launch_bounds__(256) void dz_ode_item_predict(const double* X, long long n, int d, int ld, double* like,    \
                                                                         const void* data, double* out, long long out_ld)              \
    {                                                                                                                                    \
        const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;                                                            \
        if (w >= n) return;                                                                                                              \
        const double* hdr = (const double*)data;                                                                                         \
        const long long C = (long long)hdr[0], stride = (long long)hdr[1], i = w / C;                                                    \
        const double* blk = hdr + 2 + (w - i * C) * stride;                                                                              \
        DZODE_FENCE(blk);                                                                                                                \
        double xv[dzode::view_doubles<NET>()];                                                                                           \
        const double* x = dzode::viewed_row<NET>(X + i * ld, blk, stride, xv);                                                           \
        const double v = dzode::integrate_point<dzode::OneLane<NET>>(x, blk, out + w * out_ld, nullptr, w == i * C);                     \
        like[w] = v;                                                                                                                     \
        dzode::predict_finish(v, blk, NET::O, out + w * out_ld);                                                                         \
    }
#else
#define DZODE_ENTRIES(NET)                                                                                                              \
    typedef dzode::OneLane<NET> DzodeOneLane;                                                                                            \
    DZODE_HOST_ENTRIES(DzodeOneLane)
#define DZODE_ITEM_ENTRIES(NET)                                                                                                         \
    typedef dzode::OneLane<NET> DzodeOneLane;                                                                                            \
    DZODE_HOST_ITEM_ENTRIES(DzodeOneLane)
#endif
