// certfhe/UInt.h -- EXTENSION (not in the reference): encrypted unsigned integers as bit-planes over CiphertextBatch.
//
// A w-bit value is w planes: plane j is bit j, least significant first, and each plane is a CiphertextBatch of
// `size()` elements.  Every operation is a composition of the reference's operator+ / operator* with the ONE term of
// Gates.h, in exactly this order, so its words are pinned the same way the gates are (include/csgn_hip.h, the table
// of csgn_uint_step):
//     a + b              ADD_HALF on plane 0, ADD_FULL on planes 1..w-1 (the last computes no carry)   mod 2^w
//     a - b              nb_j = logicNot(b_j), carry ONE, ADD_FULL on every plane: a + ~b + 1          mod 2^w
//     equalTo(a, b)      e = logicXnor(a_0, b_0), then EQ_STEP on planes 1..w-1
//     lessThan(a, b)     LT_FIRST on plane 0, then LT_STEP: l = logicMux(a_j + b_j, b_j, l)
//     notEqualTo         logicNot(equalTo(a, b))
//     greaterThan        lessThan(b, a)
//     lessEqual          logicNot(lessThan(b, a))
//     greaterEqual       logicNot(lessThan(a, b))
//     select(s, a, b)    logicMux(s, a_j, b_j) on every plane                                          s ? a : b
// a.add(b, &carry) and a.sub(b, &carry) also hand out the carry that leaves the top plane (the last ADD_FULL's output 1):
// the bit a widening add or a multi-word sum needs; the carry of sub decrypts to 1 where a >= b.
//
// SIZES GROW WITH WIDTH -- the scheme's own nature: with fresh 1-term planes the top plane of a sum has 2^(w-1) + 1
// terms, an equality 3^w and a less-than 3^w - 1 (at N=1247, 160 bytes a term: an 8-bit equality is about 1 MB per
// element).  compact() shrinks planes by their duplicate terms.  Every operation computes every step's size before it
// launches anything; a step above 2^31 words per element throws std::invalid_argument, and nothing is allocated.
//
// COMPARISONS WITH A PUBLIC CONSTANT (k < 2^width, the same for every element; std::invalid_argument otherwise) take k
// as plaintext instead of as a trivially encrypted UIntBatch::constant, so no term is spent on k: with fresh planes an
// equality has 2^(zeros of k) terms instead of 3^w, a less-than at most 2^w instead of about 3^w.  Their words are the
// table of csgn_uint_plain (include/csgn_hip.h), with n_j = logicNot(a_j):
//     equalTo(a, k)       g_j = k_j ? a_j : n_j;  e = g_0 * g_1 * ... * g_{w-1}  (left to right)
//     lessThan(a, k)      k == 0: ZERO; else l = n_m (m: lowest set bit), then k_j ? (l * a_j) + n_j : l * n_j
//     greaterThan(a, k)   k == 2^w-1: ZERO; else l = a_m (m: lowest clear bit), then k_j ? l * a_j : (l * n_j) + a_j
//     notEqualTo, lessEqual, greaterEqual   logicNot of equalTo, greaterThan, lessThan
// Uniform planes take one csgn_uint_plain call (one kernel for the whole comparison); ragged ones are composed from the
// CiphertextBatch operators and Gates.h.  The result's size is checked before anything is allocated or launched.
//
// PUBLIC LOOKUP TABLES: LookupTable compiles a table f of 2^inWidth entries (each < 2^outWidth; inWidth 1..16, outWidth
// 1..64) to its algebraic normal form, the Mobius transform of the table, kept on the host.  lookup(a, f) returns f(a)
// with output bit j = the sum, ascending in S, of the monomials a_{i1} * a_{i2} * ... (ascending i; ONE for the empty S)
// with bit j of anf[S] set, ZERO when there is none: csgn_uint_lut_apply's words (include/csgn_hip.h).  With fresh
// planes output j has |ANF(f_j)| <= 2^w terms.  lookup(a, b, f) indexes f by a + (b << a.width()): encrypted x
// encrypted functions of small widths (4x4-bit multiply, min, max).  Uniform planes take one csgn_uint_lut_apply (one
// launch for every output bit), its device plan cached in the LookupTable per vector of plane term counts; ragged
// planes are composed from the CiphertextBatch operators with the same words.  Every output's size is checked before
// anything is allocated; past 2^31 words per element std::invalid_argument is thrown.
//
// ENCRYPTED TABLES AT ENCRYPTED INDICES: readAt(table, index) reads a table of n = table.size() encrypted rows
// (1 <= n <= 2^v, v = index.width() <= 16) at every element's encrypted index.  Output plane j is the left-nested sum,
// ascending in r < n, of equalTo(index, r) * (plane j of row r, broadcast): the EQ row of csgn_uint_plain with k = r as
// the LEFT operand, csgn_uint_read's words (include/csgn_hip.h).  It decrypts to table[x] where x < n and to 0 in every
// plane where x >= n.  Plane j of the result has t_j * E terms, E = sum over r < n of prod_k (r_k ? s_k : s_k + 1) for
// index planes of s_k terms: 3^v with fresh planes and a full table -- 6561 at v = 8, about 1 MB per output plane and
// element at N=1247 -- the same growth as an equality.  Uniform planes take one csgn_uint_read (one launch for every
// output plane); ragged planes are composed from the CiphertextBatch operators, equalTo(index, r) and broadcast, with
// the same words.  Every size is checked before anything is allocated: std::invalid_argument for a mismatched context,
// a table of 0 or more than 2^v rows, or an output plane past 2^31 words per element.
//
// ENCRYPTED TABLES BY ENCRYPTED KEY: readWhere(keys, values, query) looks a table of n = keys.size() rows up by every
// element's encrypted query, the keys encrypted too (v = keys.width() = query.width() <= 16; values.size() = n >= 1,
// with no bound on n but the sizes): a private key-value lookup, a join, an associative memory.  Output plane j is the
// left-nested sum, ascending in r < n, of equalTo(key row r broadcast, query) * (plane j of value row r, broadcast) --
// the key as a, the query as b, the equality the LEFT operand -- and matches(keys, query), or the `member` argument,
// the sum of the equalities alone: csgn_uint_find's words (include/csgn_hip.h).  Element e decrypts to the XOR of
// values[r] over the rows with keys[r] == query[e]: with distinct keys the matching value, or 0 when no key matches.
// Rows with EQUAL KEYS XOR their values, and member is the PARITY of the number of matching rows -- membership only
// when the keys are distinct.  Plane j of the result has n * P * t_j terms, P = prod_k (u_k + s_k + 1) for key planes of
// u_k and query planes of s_k terms: n * 3^v with fresh planes (6561 n at v = 8), the same growth as an equality per row.
// Uniform planes take one csgn_uint_find (one launch for every output plane and member); ragged planes (a compact()
// result on any operand) are composed from slice, broadcast, equalTo(a, b), * and + with the same words.  Every size is
// checked before anything is allocated: std::invalid_argument for mismatched contexts, keys.width() != query.width(), a
// width past 16, keys.size() != values.size(), no rows, or an output past 2^31 words per element.  An empty query batch
// gives empty planes.
//
// ENCRYPTED ARRAYS WRITTEN AT ENCRYPTED INDICES: writeAtEach(arrays, n, index, value) returns the arrays of readAtEach's
// layout (element e owns rows e * n .. e * n + n - 1) with row index[e] of array e replaced by value[e]: a private
// counter table, an oblivious register file, one step of an oblivious RAM, a per-record field update.  Element e * n + r
// of plane j is logicMux(equalTo(index, r), value_j, arrays_j) = (EQ * (value + d)) + d on elements e and e * n + r --
// the EQ row of csgn_uint_plain with k = r as the LEFT operand -- csgn_uint_write's words (include/csgn_hip.h).  It
// decrypts to the arrays, with value[e] in row index[e] where index[e] < n.  Row r has P_r * (tv + td) + td terms for
// value planes of tv and array planes of td terms, P_r the terms of equalTo(index, r) (fresh planes: 2^zeros(r)), so
// the result's planes are RAGGED CiphertextBatches in a pattern of period n; their offsets are computed on the host
// (csgn_uint_write_offset), with no device round trip, and termsOf(e * n + r) gives each row's size.  Everything that
// takes ragged planes reads them back: readAtEach(writeAtEach(a, n, i, x), n, i) decrypts to x where i < n.
// THE READ THAT FOLLOWS: readAtEach over planes whose terms have period n -- termsOf(e * n + r) == termsOf(r) for every
// e, which is what writeAtEach returns; a uniform plane has it with a constant -- under a uniform index of at most 16
// bits is one csgn_uint_pick_rows (include/csgn_hip.h): one launch for every plane, straight from the written planes,
// and the result's planes are UNIFORM CiphertextBatches (sum over r of P_r * termsOf(r) terms an element), with the
// words, in the order, that the class-level loop over the same operands gives.  Its sizes are checked on the host
// (csgn_uint_pick_rows_check) before anything is allocated.  readAtEachRoute names the route.
// writeAt(table, index, value) is the same for ONE index and value and n = table.size().  Uniform operands under an
// index of at most 16 bits take one csgn_uint_write (one launch for every plane, the rows' raw copies included);
// ragged operands (a compact() result) and wider indices are composed from equalTo(index, r), gather, logicMux, concat
// and a permuting gather, with the same words.  Every size is computed before anything is allocated:
// std::invalid_argument for mismatched contexts, widths or counts, n of 0 or past 2^index.width(), arrays.size() !=
// n * index.size(), or an array past 2^31 words.  An empty batch gives empty planes.
//
// ARITHMETIC WITH A PUBLIC CONSTANT (k < 2^width, the same for every element; std::invalid_argument otherwise) spends no
// term on k: with m the lowest set bit of k the carry into plane j > m is the chain c_m = a_m, then k_j ? (c * n_j) + a_j
// : c * a_j (n_j = logicNot(a_j), c the LEFT operand), and the words are csgn_uint_addk's (include/csgn_hip.h):
//     a + k              k == 0: a copy.  out_j = a_j (j < m), a_m + ONE, then k_j ? (a_j + c) + ONE : a_j + c  mod 2^w
//     a.add(k, &carry)   the same planes, and the c left after the top plane (ZERO when k == 0)
//     a - k              a + ((2^w - k) mod 2^w)
//     k - a              logicNot of every plane of a + (~k mod 2^w)
//     -a                 0 - a: logicNot of every plane of a + (2^w - 1)
//     ~a                 logicNot(a_j) on every plane
// With fresh planes plane j of a + 1 has 2 terms (a_j + a_0 * ... * a_{j-1}) where a + constant(1) has 2^j + 1; in
// general the carry has at most 2^(set bits of k from m to j) - 1 terms.  Uniform planes take one csgn_uint_addk call
// (one kernel for every plane and the carry-out); ragged ones are composed from the CiphertextBatch operators and
// Gates.h with the same words.  Every plane's size is checked before anything is allocated.
//
// A PUBLIC CONSTANT WHERE AN ENCRYPTED FLAG IS SET (k < 2^width, the same for every element; std::invalid_argument
// otherwise): addWhere(mask, a, k) is a + (mask ? k : 0) mod 2^w -- a private counter hits += [key == q], a vote, a
// conditional accumulation of a public amount, the carry-in of an add, a conditional + 1.  It spends terms only where k
// has a set bit: the ADD chain of a + b with b_j = mask where k_j = 1 and NO b_j where k_j = 0, csgn_uint_add_where's
// words (include/csgn_hip.h).  With m the lowest set bit of k:
//     addWhere(mask, a, k)       k == 0: the planes of a themselves (the same payloads).  out_j = a_j (j < m), a_m + mask
//                                (c = a_m * mask), then k_j ? (a_j + mask) + c : a_j + c, with the carry
//                                k_j ? (a_j * mask) + ((a_j + mask) * c) : a_j * c
//     ..., &carry)               the same planes, and the c left after the top plane (ZERO when k == 0)
//     subWhere(mask, a, k)       addWhere(mask, a, (2^w - k) mod 2^w); its carry is no borrow and is not offered
//     incrementWhere(mask, a)    k = 1                decrementWhere(mask, a)    k = 2^w - 1
// Sizes, fresh a and mask, all planes and the carry together (through a + keepWhere(mask, constant): 518 at w = 8, 131 086
// at w = 16, and nothing past 16 planes):
//     w = 8, k = 1      17 (2 a plane, carry 1)              w = 8, k = 0x64    31 (1,1,2,2,2,3,5,8; carry 7)
//     w = 8, k = 0xFF   518 (2,3,5,9,17,33,65,129; 255)      w = 16, k = 1      33              w = 32, k = 1      65
// Uniform operands of width <= 32 take ONE csgn_uint_add_where (one launch for every plane and the carry) -- but for
// the shape class the launch lost to the loop's launches in DESIGN 4.35 (0.6 of their speed): one-term planes and mask
// under a k of ONE set bit with 16 planes or more above it, at 256 MiB of outputs or more, which stays on the loop; a
// ragged mask or plane (a compact() result) and widths 33..64 take the loop too, the table above through CiphertextBatch::operator+ / operator* in exactly
// its order, with the same words.  Knob uint_add_where_form (csgn_set_tuning, or CSGN_UINT_ADD_WHERE_FORM when the
// library loads) forces the loop (0) or the call where it can run (1); addWhereRoute names the route.  Every size is
// computed before anything is allocated: std::invalid_argument for mismatched contexts or counts, k >= 2^w, or an output
// past 2^31 words per element.  An empty batch gives empty planes.
//
// PUBLIC LINEAR MAPS OVER F2.  linearMap(a, m, constant) applies the public matrix m (class F2Matrix: one 64-bit row
// mask over a's planes per output plane) to every element and XORs the public constant: SHA-2's sigma functions, an
// xorshift step, Gray codes, CRC steps, AES MixColumns, a carry-less product or a product in GF(2^w) with a public
// factor, a masked parity.  No ciphertext is multiplied: csgn_uint_linear's words (include/csgn_hip.h),
//     plane j = ((a_{i1} + a_{i2}) + ...) + a_{im} [+ ONE where constant_j = 1],   i1 < i2 < ... the set bits of row j
// so a row of m bits over fresh planes has m (+ 1) terms, where the chain a.rotateRight(7) ^ a.rotateRight(18) ^ ...
// copies the running sum once per link and takes m - 1 launches.  What is PUBLIC cancels before anything runs:
// F2Matrix::operator* composes two maps over F2 and operator^ adds them, so a term two branches both contribute is gone
// from the matrix (grayDecode(w) * grayEncode(w) IS identity(w)), where the chain keeps it in the ciphertext twice.
// A row of exactly one bit and no constant returns the SAME payload as the source plane, as the public shifts do; a
// zero row returns the constant batch (ZERO, or ONE under a constant bit); such rows are left out of the call, and if
// nothing is left nothing is launched.  Uniform planes take ONE csgn_uint_linear for all other rows (k_uint_linear,
// DESIGN 4.36); a ragged plane (a compact() result) takes the loop, the same table through CiphertextBatch::operator+
// and the constant batches, with the same words.  linearRoute names the route.  Every size is computed before anything
// is allocated or launched: std::invalid_argument for a.width() != m.inWidth(), a constant of outWidth() bits or more,
// or an output past 2^31 words per element.  An empty batch gives empty planes.  parity(a, mask) is the one-row map.
//
// PUBLIC BILINEAR FORMS OVER F2 OF TWO ENCRYPTED INTEGERS.  bilinearMap(a, b, form, constant) evaluates the public form
// (class F2Bilinear: per output plane the list of pairs (i, l) whose products a_i * b_l are summed) on every element and
// XORs the public constant: clmul(a, b), the step of GHASH / POLYVAL and of every polynomial MAC; gfMul(a, b, poly), the
// product in GF(2^w) (AES's inversion as x^254, Reed-Solomon, Shamir shares over GF(256)); a secret bit matrix applied
// to a secret vector; dotBits(a, b) = parity(a & b).  No carry exists: csgn_uint_bilinear's words (include/csgn_hip.h),
//     plane j = ((a_i1 * b_l1 + a_i2 * b_l2) + ...) + a_im * b_lm [+ ONE where constant_j = 1]
// the pairs of row j ascending by (i, l), so over fresh planes a row of m pairs has m (+ 1) terms.  What is PUBLIC
// cancels before anything runs: F2Bilinear keeps every row sorted with nothing twice, F2Matrix * F2Bilinear applies a
// linear map after the form and F2Bilinear::compose applies linear maps to its arguments, so gfMul(w, poly) IS the
// reduction matrix times clmulWide(w).  Squaring in GF(2^w) is LINEAR (F2Matrix::gfSquare, through linearMap): an
// inversion chain multiplies only where it must.  A row of no pair is the constant batch (ZERO, or ONE under a constant
// bit).  Uniform planes take ONE plan, cached for the process like the csgn_uint_plain_sum plans, and ONE
// csgn_uint_bilinear for all planes (k_uint_bilinear); a ragged plane (a compact() result) takes the loop:
// two concat, then per output plane two gather, ONE operator* and sumGroups, with the same words.  bilinearRoute names the
// route.  Every size is computed before anything is allocated or launched: std::invalid_argument for widths that are
// not the form's, operands of different counts or contexts, a constant of outWidth() bits or more, or an output past
// 2^31 words per element.  An empty batch gives empty planes.
//
// PUBLIC POLYNOMIAL MAPS OVER F2.  polyMap(operands, f, constant) evaluates the public polynomial f (class
// F2Polynomial: per output plane a set of monomials, each a set of bits of the operands) on every element and XORs the
// public constant: a sparse polynomial of mixed degree up to 8 over several integers of 256 bits in all -- SHA-2's
// Ch(e, f, g) = ef + eg + g and Maj(a, b, c) = ab + ac + bc, Keccak's chi a + c + bc, a Simon round, a full adder's
// carry, a k-way AND, a & b & ~c, a gfMul plus an affine term, an S-box ANF with few monomials.  No carry exists:
// csgn_uint_poly's words (include/csgn_hip.h) over the operands' planes concatenated in order,
//     plane j = ((M_1 + M_2) + ...) + M_m [+ ONE where constant_j = 1],   M = ((p_f1 * p_f2) * ...) * p_fd
// the monomials of row j ascending by (degree, then the factor list), the factors of a monomial ascending:
//     form                   terms of a plane over fresh planes        over planes of t terms
//     ch, maj, chi           3                                         ch 2 t^2 + t, maj 3 t^2, chi 2 t + t^2
//     andAll of k operands   1                                         t^k
//     mux                    3                                         2 t^2 + t (s of t terms too)
//     a monomial of degree d 1                                         t^d: degree 8 of 2-term planes has 256
// What is PUBLIC cancels before anything runs: a monomial named an even number of times is gone, and a variable named
// twice inside a monomial is named once (x x = x is an identity of the function; the C ABI would multiply the plane with
// itself, t^2 terms: the words differ, the value does not).  F2Polynomial::linear(m) has exactly linearMap's words and
// F2Polynomial::bilinear(f) exactly bilinearMap's.  A row that is exactly one monomial of degree 1 with no constant
// returns the SAME payload as the source plane; a row of no monomial is the constant batch (ZERO, or ONE under a constant
// bit); such rows are left out of the call, and if nothing is left nothing is launched.  Uniform planes take ONE plan,
// cached for the process like the csgn_uint_bilinear plans, and ONE csgn_uint_poly for all other rows (k_uint_poly,
// DESIGN 4.39); a ragged plane (a compact() result) takes the loop: one concat of all operand planes, then per output
// plane and per degree d present, ascending, d gather, d - 1 operator* and sumGroups, operator+ between the degree
// groups, + ONE, with the same words.  polyRoute names the route.  Every size is computed before anything is allocated or
// launched: std::invalid_argument for widths or counts that are not the form's, operands of different counts or
// contexts, a constant of outWidth() bits or more, or an output past 2^31 words per element.  An empty batch gives empty
// planes.
//
// RANGES, SETS AND STEP FUNCTIONS OF PUBLIC CONSTANTS.  Over F2 they are sums (operator+, concatenation) of the
// comparisons above of ONE integer, plus at most one ONE: csgn_uint_plain_sum's words (include/csgn_hip.h).  With
// P(cmp, k) the words of the comparison of a with the public k (lessThan(a, k) is P(LT, k), ...), top = 2^w - 1:
//     inRange(a, lo, hi)      lo == 0 and hi == top: the constant ONE;  lo == 0: lessEqual(a, hi)'s words;
//                             hi == top: greaterEqual(a, lo)'s words;  otherwise P(LT, hi + 1) + P(LT, lo)
//     outOfRange(a, lo, hi)   inRange's words followed by + ONE (over the full range that is ONE + ONE, two terms)
//     inRanges(a, intervals)  the sum, in order, of the inRange entries of the disjoint ascending intervals
//                             [lo_0, hi_0], [lo_1, hi_1], ... (hi_i < lo_{i+1}); a full interval [0, top] is + ONE
//     isIn(a, set)            the sum of P(EQ, k_i) over the distinct values of the set, ascending (sorted and
//                             deduplicated on the host: a duplicate would cancel over F2); notIn: followed by + ONE
//     stepFunction(a, thresholds, values, out_width)
//                             thresholds 0 < t_1 < ... < t_m <= top and m + 1 values below 2^out_width: the result is
//                             v_i where t_i <= a < t_{i+1} (v_0 below t_1).  Plane j is the sum, ascending in i, of
//                             P(LT, t_i) over the i with bit j of v_{i-1} ^ v_i set, + ONE where bit j of v_m is set
//     bucketOf(a, thresholds, planes)    the step function with the values 0, 1, ..., m: the index of a's bucket
//     lookupSparse(a, keys, values, out_width, otherwise)
//                             values[i] where a == keys[i] (the first of equal keys counts), `otherwise` elsewhere.
//                             Plane j is the sum, over the distinct keys ascending, of P(EQ, k_i) where bit j of
//                             v_i ^ otherwise is set, + ONE where bit j of otherwise is set: a public table on integers
//                             of any width whose cost grows with the number of keys, not with 2^w
// A plane of no entry is the constant batch (ZERO, or ONE); a plane that is exactly one comparison is that comparison's
// call (csgn_uint_plain); uniform planes take ONE plan and ONE csgn_uint_plain_sum (k_uint_plain_sum) for
// all other planes, the plan cached for the process like the csgn_wsum plans; a ragged plane takes the definition
// through the batch operators, as the comparisons do.  plainSumRoute names the route.  Every size is computed by the
// host-only entry points before anything is allocated or launched: std::invalid_argument for lo > hi, a bound, key or
// threshold of 2^w or more, intervals or thresholds out of order, a threshold of 0, a wrong number of values, a value
// of 2^out_width or more, out_width outside 1..64, or an output past 2^31 words per element.  An empty batch gives
// empty planes.
//
// BITWISE OPERATORS AND SHIFTS.  Between two integers of one width, context and count, per plane:
//     a & b              a_j * b_j            a | b     logicOr(a_j, b_j)            a ^ b     a_j + b_j
// With a public constant (k < 2^width) and for a public distance s nothing is computed on ciphertext words beyond a
// logicNot; a kept plane is the SAME immutable payload as the source's, not a copy:
//     a & k              a_j where k_j = 1, ZERO (one term, constantBatch) elsewhere
//     a | k              ONE (constantBatch) where k_j = 1, a_j elsewhere
//     a ^ k              logicNot(a_j) where k_j = 1, a_j elsewhere
//     a.shiftLeft(s)     plane j = a_{j-s} for j >= s, ZERO below; every plane ZERO when s >= width
//     a.shiftRight(s)    plane j = a_{j+s} for j + s < width, ZERO above; every plane ZERO when s >= width
//     a.rotateLeft(s)    plane j = a_{(j - s) mod width}, s taken mod width
//     a.rotateRight(s)   rotateLeft(width - s mod width)
//
// SHIFTS, ROTATES AND OWN ARRAYS BY ENCRYPTED AMOUNTS: a.shiftLeft(d), shiftRight(d), rotateLeft(d), rotateRight(d) move
// every element by ITS OWN encrypted distance d (one context and count; v = d.width()), and readAtEach(arrays, n, index)
// reads, for element e, row index[e] of the n rows e * n .. e * n + n - 1 of `arrays`: x << (y & 31), the data-dependent
// rotations of RC5-style ciphers, a barrel shifter, a per-record array, n-way selection.  Output plane j is the
// left-nested sum, ascending in r < rows_j, of equalTo(d, r) * (a source plane of the same element) -- the EQ row of
// csgn_uint_plain with k = r as the LEFT operand -- csgn_uint_pick's words (include/csgn_hip.h):
//     a.shiftLeft(d)     rows_j = min(j + 1, 2^v), source a_{j-r}           (a << d) mod 2^w, 0 where d >= w
//     a.shiftRight(d)    rows_j = min(w - j, 2^v), source a_{j+r}           a >> d, 0 where d >= w
//     a.rotateLeft(d)    rows_j = 2^v, source a_{(j-r) mod w}               a rotated left by d mod w
//     a.rotateRight(d)   rows_j = 2^v, source a_{(j+r) mod w}               a rotated right by d mod w
//     readAtEach         rows_j = n, source plane j of element e * n + r    arrays[e * n + index[e]], 0 where index[e] >= n
// Plane j has t * E_j terms for source planes of t terms, E_j the terms of readAt's E over rows_j rows: with fresh planes
// the top plane of an 8-bit shiftLeft by a 3-bit distance has 27 terms, a plane of a 32-bit rotate by 5 bits 243.
// Uniform planes of ONE term count under a distance of at most 16 bits take one csgn_uint_pick (one launch for every
// output plane); ragged planes (a compact() result), planes of different term counts and wider distances are composed
// from equalTo(d, r), operator*, left-nested operator+ and, for readAtEach, gather, with the same words.  Every size is
// computed before anything is allocated: std::invalid_argument for mismatched contexts or counts, n of 0 or past
// 2^index.width(), arrays.size() != n * index.size(), or an output past 2^31 words per element.  An empty batch gives
// empty planes.
//
// COUNTING: countOnes(bits, g, planes) counts the ones among every g consecutive elements of a batch of encrypted bits
// into an encrypted integer, modulo 2^planes: COUNT(*) of matching rows, the Hamming weight of a word, the Hamming
// distance of two words.  Bit j of the number of ones among g bits is the elementary symmetric polynomial of degree
// m = 2^j over F2, so plane j is the left-nested sum, over the m-subsets i_1 < ... < i_m of the group in lexicographic
// order (the nested loops), of the left-nested products x_{i_1} * ... * x_{i_m}: csgn_count's words
// (include/csgn_hip.h).  Plane j has C(g, m) * t^m terms for inputs of t terms: with g = 64 fresh bits 64, 2016 and
// 635 376 terms for planes 0, 1, 2; planes 3, 4, 5 are past any memory, and plane 6 is one term, the AND of all 64 --
// so countBit / popcountBit name ONE plane.  A plane with 2^j > g is the one-term ZERO of constantBatch.  Plane 0 is
// sumGroups(g): it shares the payload and costs no launch; the other planes of a uniform batch come from ONE csgn_count
// (one launch), as does every plane of popcount when all planes of `a` are uniform with one term count.  Ragged
// operands, or planes of different term counts, are composed from gather, operator* and sumGroups with the same words.
// Every size is computed before anything is allocated or launched: std::invalid_argument for a group of 0 or one that
// does not divide size(), `planes` of 0 or above 64, mismatched contexts or widths, or a plane past 2^31 words per
// element.  An empty batch gives empty planes.
//
// RUNNING COUNTS: runningCount(bits, g, planes) returns g integers, entry r the number of ones among the group's rows
// 0..r (with `exclusive`: among the rows before r) -- a cumulative count, the rank of a row among the matching rows, the
// segment number of a row from "a segment starts here" flags; runningCountBit names one plane (j = 0: the running
// parity) and prefixPopcount(a, planes) is the rank function of an integer's own bits.  Entry r has word for word the
// planes of countOnes over the gathered rows: C(n_r, 2^j) * t^(2^j) terms with n_r = r + 1 - exclusive, and the
// one-term ZERO of constantBatch where 2^j > n_r.  Uniform inputs of one term count take ONE csgn_count_prefix
// (include/csgn_hip.h; one launch): it writes one block a plane, the rows of all g entries one after the other, and
// the entries are views that keep the block alive -- 16 fresh flags: 136, 681, 6191, 24 317 and 16 terms per element
// for planes 0 to 4.  Planes with 2^j > g - exclusive are ZERO without a launch.  Ragged operands, or inputs of
// different term counts, take the definition's loop: the gathered prefix through countOnes' route, row by row, with
// the same words.  runningCountRoute names the route.  Every size is computed before anything is allocated or
// launched: std::invalid_argument as for countOnes, the size that of the last row.  An empty batch gives empty planes.
//
// SUMS: sumValues(a, g, planes) adds every g consecutive integers of a batch into an encrypted integer modulo
// 2^planes, sumWhere(mask, values, g, planes) only those whose encrypted mask bit is set (SUM(value) of the matching
// rows), mul(a, b, planes) multiplies two encrypted integers and innerProduct(a, b, g, planes) adds g products.  All are
// one weighted sum of encrypted bits (include/csgn_hip.h, csgn_wsum): class c holds the bits of weight 2^c -- plane c of
// the g rows; mask * values.plane(c); the partial products a_i * b_{c-i}, i ascending, a on the left; those of every
// row, row slowest -- and bit j of the sum is the sum, over the count vectors (m_j .. m_0) with sum m_c 2^c = 2^j in
// ascending order and over their selections, of the product of the selected bits, classes descending: no carry is
// ever materialised.  Term counts of fresh operands, planes 0, 1, 2, ...: the sum of 4 three-bit integers 4, 10, 35,
// 161, 315; a 4 x 4 -> 8 bit product 1, 2, 4, 10, 34, 129, 383, 511.  A plane with no count vector is the one-term ZERO
// of constantBatch.  Plane 0 of sumValues is plane(0).sumGroups(g): it shares the payload and costs no launch.
// Uniform classes of one term count take ONE csgn_wsum (one launch; plans are kept per shape); ragged operands (a
// compact() result) or planes of different term counts are composed from gather, operator*, sumGroups and operator+ in
// the definition's loop order, with the same words.  Every size is computed before anything is allocated or launched:
// std::invalid_argument for a group of 0 or one that does not divide size(), `planes` of 0 or above 64, mismatched
// contexts or counts, more than 65 536 bits an element, or a plane past 2^31 words per element.  An empty batch gives
// empty planes.  Multiplication by a PUBLIC constant stays with LookupTable.
//
// ORDERING: min(a, b), max(a, b), minMax(a, b), selectLess(a, b, x, y) and compareExchange select by the ENCRYPTED
// comparison a < b: the step of every oblivious sort, top-k, median filter, arg-min and clamp.  Every output plane is
// logicMux(lessThan(a, b), x_j, y_j) = (L * (x_j + y_j)) + y_j, the comparison the LEFT operand -- the words of
// select(lessThan(a, b), x, y), csgn_uint_lt_select's (include/csgn_hip.h) -- and decrypts to x_j where a < b and to y_j
// elsewhere: A TIE TAKES y.  min pairs (a_j, b_j), max pairs (b_j, a_j); compareExchange(a, b, pa, pb, ...) gives the
// keys and the payloads that travel with them from the SAME launch: lo = min, hi = max, plo = a < b ? pa : pb,
// phi = a < b ? pb : pa; on a tie lo = b, hi = a, plo = pb and phi = pa, so equal keys keep their payloads apart.  A null
// output is skipped.  A plane of the result has L * (tx + ty) + ty terms for request planes of tx and ty terms, L the
// terms of lessThan(a, b): 3^w - 1 with fresh planes (6560 at w = 8, about 2 MB per output plane and element at
// N=1247), the same growth as a less-than.  Uniform planes of width <= 16 take one csgn_uint_lt_select per 64 output
// planes (one launch for all of them; the comparison is never written); ragged planes (a compact() result on any
// operand) or wider integers are composed from lessThan(a, b) and logicMux with the same words.  Every size is computed
// before anything is allocated: std::invalid_argument for mismatched contexts, counts or widths, or an output past 2^31
// words per element.  An empty batch gives empty planes.
//
// a + b, a - b, a.add / a.sub, equalTo(a, b) and notEqualTo(a, b) on uniform planes of width <= 16 are ONE call,
// csgn_uint_arith (include/csgn_hip.h): one launch writes every plane and the carry, each term decoded from its position,
// and no running carry or equality is ever written; lessThan(a, b) and greaterThan(a, b) take csgn_uint_lt_select with
// no requests, the comparison alone.  Wider integers and ragged planes (what compact() may return) take the chain the
// table above spells: one csgn_uint_step (or csgn_gate_uniform) call per bit on uniform planes, the CiphertextBatch
// operators and Gates.h on ragged ones, only the running carry or accumulator alive between bits -- the same words
// either way.  Knob uint_arith_form (csgn_set_tuning, or CSGN_UINT_ARITH_FORM when the library loads) forces the chain
// (0) or the one call (1); left alone (-1), a forced uint_fused keeps the chain, so that both forms of csgn_uint_step can
// be run through these operators.  arithRoute names the route.  lessEqual and greaterEqual keep the chain and logicNot.
//
// THE PLANE-BY-PLANE OPERATORS IN ONE CALL: a & b, a | b, a ^ b, ~a, a ^ k, select(s, a, b) and keepWhere(mask, a) on
// uniform planes are ONE csgn_uint_bitwise (include/csgn_hip.h) for every plane, whatever the planes' term counts:
//     keepWhere(mask, a)  mask * a_j on every plane, the mask the LEFT operand                         mask ? a : 0
// the WHERE of a query applied to a whole integer, and what sumWhere builds its classes with; a plane has ts * ta_j
// terms for a mask of ts terms.  a ^ k passes only the planes with a set bit of k; the others go on sharing the source's
// payload.  hammingDistance takes the call through a ^ b.  The C call writes all planes from one kernel or issues the
// launchers of the CiphertextBatch operators and Gates.h plane by plane, by shape and by knob uint_bitwise_form
// (csgn_set_tuning, or CSGN_UINT_BITWISE_FORM when the library loads: 0 the launchers, 1 the kernel; left alone, a forced
// gate_fused keeps the launchers, so that both forms of csgn_gate_uniform can be run through these operators).  Ragged
// planes (what compact() may return) and empty batches take the CiphertextBatch operators and Gates.h plane by plane --
// the same words on every route.  Every plane's size is checked before anything is allocated: std::invalid_argument for
// mismatched contexts, widths or counts, or a plane past 2^31 words per element; keepWhere of an empty batch gives empty
// planes.  bitwiseRoute names the route.
//
// PRIORITY: firstWhere(mask, values, g) gives, of every g consecutive rows, the value of the FIRST one whose encrypted
// mask bit is set -- the LIMIT 1 / EXISTS of a private query, first-fit, a priority encoder or arbiter; anyOf(bits, g)
// is the OR of every g bits (a true "is there any match", where matches and member are the PARITY), firstIndex the
// index of that row, and of an integer's own planes lowestSetIndex is find-first-set, lowestSetBit is a & -a and
// bitLength the position of the highest set bit plus one.  All are csgn_uint_first's words (include/csgn_hip.h): with
// n_r = logicNot(m_r),
//     F_0 = m_0,  F_r = (((n_0 * n_1) * ...) * n_{r-1}) * m_r        exactly one F_r decrypts to 1: the first set row's
//     firstWhere plane j     ((F_0 * d_{0,j}) + (F_1 * d_{1,j})) + ... + (F_{g-1} * d_{g-1,j}), F the LEFT operand
//     anyOf, *any, *nonzero  (F_0 + F_1) + ... + F_{g-1}
//     plane i of an index    the left-nested sum, ascending in r, of F_r over the rows whose PUBLIC label has bit i
// with the labels r (firstIndex, lowestSetIndex), 1 << r (lowestSetBit: plane r is F_r itself) and width - r over the
// planes taken from the top (bitLength).  Everything decrypts to 0 where no mask bit is set; *any tells.  A row of s_r
// terms has P_r = s_r * prod_{i<r} (s_i + 1) entries, the stream Q = prod_r (s_r + 1) - 1: with fresh masks P_r = 2^r and
// Q = 2^g - 1, so firstWhere over 8 fresh rows writes 255 * t terms a plane and the bit length of a fresh 16-bit integer
// 65 535 terms in all -- the scheme's own growth, much gentler than an equality's 3^v.  A label plane that no row's label
// reaches, or one past the labels' width, is the one-term ZERO of constantBatch.  Uniform operands (in the grouped
// layout: of one mask term count) take ONE csgn_uint_first, one launch for every plane, *any and the label planes;
// ragged operands (a compact() result) are composed from gather, logicNot, operator* and left-nested operator+ in the
// definition's loop order, with the same words.  firstRoute names the route.  Every size is computed before anything
// is allocated or launched: std::invalid_argument for a group of 0 or above 64 or one that does not divide size(),
// mismatched contexts or counts, `planes` of 0 or above 64, or an output past 2^31 words per element.  An empty batch
// gives empty planes.
//
// SELECTION BY RANK: nthWhere(mask, values, g, s) gives, of every g consecutive rows, the value of the (s + 1)-th one
// whose encrypted mask bit is set -- LIMIT k / OFFSET s of a private query, the oblivious compaction of the matching
// rows to the front (takeWhere: slots 0 .. k-1), select_k on a bit vector; nthIndex is the index of that row and
// nthSetIndex the position of the (s + 1)-th set bit of an integer; atLeast(bits, g, k) is "at least k of every g bits
// are set" -- HAVING COUNT(*) >= k, k-of-n voting -- without the count planes and the comparison that countOnes and
// lessThan would spend on it, and popcountAtLeast(a ^ b, k) the Hamming-distance threshold (hammingDistance(a, b) <= r
// is logicNot(popcountAtLeast(a ^ b, r + 1))).  All are csgn_uint_nth's words (include/csgn_hip.h): with [x] for "x is
// odd", for a row r >= s
//     G_{r,s} = the left-nested sum, over d ascending in s..r with [C(d, s)] and over the d-subsets i_1 < ... < i_d of
//               the rows below r in lexicographic order, of (((m_{i_1} * m_{i_2}) * ...) * m_{i_d}) * m_r
//     nthWhere plane j     ((G_{s,s} * d_{s,j}) + (G_{s+1,s} * d_{s+1,j})) + ... + (G_{g-1,s} * d_{g-1,j}), G the LEFT operand
//     atLeast, *valid      (G_{s,s} + G_{s+1,s}) + ... + G_{g-1,s}                     (atLeast(bits, g, k): s = k - 1)
//     plane i of an index  the left-nested sum, ascending in r >= s, of G_{r,s} over the rows whose PUBLIC label has bit i
// ("exactly s of the rows above r are set" is symmetric, so its ANF is the sum of the elementary symmetric polynomials
// e_d with [C(d, s)]).  Exactly one G_{r,s} decrypts to 1 when more than s mask bits are set: the (s + 1)-th set row's;
// everything decrypts to 0 otherwise, and *valid tells.  Every row has the same t terms in one call; the stream has
// Q_s = sum over d with [C(d, s)] of C(g, d+1) * t^(d+1) entries: fresh masks of 8 rows give 255, 127, 135, 71, 93, 29,
// 9, 1 for s = 0..7, Q_0 = 2^g - 1 is firstWhere's count, and the HIGH slots of wide groups stay small (65 entries for
// the 63rd set bit of a fresh 64-bit integer) while the low slots of wide groups are past any memory and are refused.
// atLeast(bits, g, 0) is the one-term ONE and atLeast(bits, g, k > g) the one-term ZERO of constantBatch, as is a label
// plane no row from the slot on reaches.  Uniform operands whose mask rows have one term count take ONE csgn_uint_nth
// per slot, one launch for every plane, *valid and the label planes; ragged operands (a compact() result) and rows of
// different term counts are composed from gather, operator* and left-nested operator+ in the definition's loop order,
// with the same words.  nthRoute names the route.  Every size is computed before anything is allocated or launched:
// std::invalid_argument for a group of 0 or above 64 or one that does not divide size(), slot >= group, a k of
// takeWhere of 0 or above the group, `planes` of 0 or above 64, mismatched contexts or counts, or an output past 2^31
// words per element.  An empty batch gives empty planes.
//
// THE TWO ENDS.  UIntBatch::encrypt (both overloads) makes ONE block of width * count ciphertexts, lays the bit bytes
// plane after plane in one host pass, uploads them once and runs one csgn_encrypt_keyed from stream position 0; plane j
// is a VIEW at word j * count * dL of that block, so a plane -- also one handed on by plane(j) after the UIntBatch is
// gone -- keeps the whole block alive.  The seeded planes are word for word CiphertextBatch::encrypt(key, bits_j, seed,
// j * count).  With count * dL odd the views would sit on 8-byte boundaries and put every later kernel on its 8-byte
// path, so such a batch is encrypted plane by plane, each plane a block of its own.  UIntBatch::decrypt is
// decryptPacked(planes, key): one csgn_uint_decrypt (include/csgn_hip.h) reads every term of every plane once and
// writes one word per element, then one copy of 8 bytes per element to the host and one synchronisation.  Knob
// uint_decrypt_form (csgn_set_tuning, or CSGN_UINT_DECRYPT_FORM when the library loads) at 0 keeps one
// CiphertextBatch::decrypt per plane, which is also what a ragged plane with an element of more than 4096 terms makes
// the whole list take; decryptRoute names the route.  The values are the same.
#ifndef CERTFHE_UINT_H
#define CERTFHE_UINT_H

#include <stdint.h>

#include <memory>
#include <utility>
#include <vector>

#include "Batch.h"
#include "Context.h"
#include "SecretKey.h"

namespace certFHE {

class UIntBatch {
    std::vector<CiphertextBatch> planes_;
    explicit UIntBatch(const std::vector<CiphertextBatch> &planes);

  public:
    // values[i] < 2^width, width in 1..64 (std::invalid_argument otherwise).  Plane j encrypts bit j of every value.
    static UIntBatch encrypt(const SecretKey &key, const std::vector<uint64_t> &values, unsigned width);
    // REPRODUCIBLE form (tests, benchmarks): plane j is CiphertextBatch::encrypt(key, bits_j, seed, j * values.size())
    static UIntBatch encrypt(const SecretKey &key, const std::vector<uint64_t> &values, unsigned width, uint64_t seed);
    // trivial encryptions (Gates.h constantBatch per plane): their values are public
    static UIntBatch constant(const Context &context, const std::vector<uint64_t> &values, unsigned width);
    // planes[j] is bit j; 1..64 planes of one context and element count
    static UIntBatch fromPlanes(const std::vector<CiphertextBatch> &planes);

    const CiphertextBatch &plane(unsigned j) const;   // std::out_of_range past width()
    unsigned width() const { return (unsigned)planes_.size(); }
    uint64_t size() const { return planes_[0].size(); }
    const Context &context() const { return planes_[0].context(); }
    UIntBatch compact() const;                          // CiphertextBatch::compact on every plane
    std::vector<uint64_t> decrypt(const SecretKey &key) const;

    // modulo 2^width; both operands of one width, context and element count
    // The data movement of CiphertextBatch (Batch.h) on every plane: element e of the result is a bit-for-bit copy of a
    // source integer.  gather and broadcast move every uniform plane in ONE launch (csgn_gather_planes); ragged planes
    // go through CiphertextBatch::gather / broadcast.  gather: std::out_of_range before anything is allocated;
    // slice: std::out_of_range unless begin <= end <= size(); broadcast: std::invalid_argument unless size() == 1;
    // concat: std::invalid_argument for no parts, or parts of different widths or contexts.
    UIntBatch gather(const std::vector<uint64_t> &indices) const;
    UIntBatch slice(uint64_t begin, uint64_t end) const;
    UIntBatch broadcast(uint64_t count) const;
    static UIntBatch concat(const std::vector<UIntBatch> &parts);

    UIntBatch operator+(const UIntBatch &rhs) const;
    UIntBatch operator-(const UIntBatch &rhs) const;
    // a + b and a - b with the carry that leaves the top plane, for every width and for ragged planes (carry_out may
    // be null: the same as the operators).  The carry of add decrypts to 1 where a + b >= 2^width, that of sub
    // (a + ~b + 1) to 1 where a >= b.
    UIntBatch add(const UIntBatch &rhs, CiphertextBatch *carry_out) const;
    UIntBatch sub(const UIntBatch &rhs, CiphertextBatch *carry_out) const;
    // a * b modulo 2^width: mul(*this, rhs, width())
    UIntBatch operator*(const UIntBatch &rhs) const;

    // with the public constant k < 2^width (std::invalid_argument otherwise), modulo 2^width
    UIntBatch operator+(uint64_t k) const;
    UIntBatch operator-(uint64_t k) const;
    friend UIntBatch operator-(uint64_t k, const UIntBatch &a);     // k - a
    UIntBatch operator-() const;                                    // -a
    // a + k and the bit that left (carry_out may be null: the same as operator+)
    UIntBatch add(uint64_t k, CiphertextBatch *carry_out) const;

    UIntBatch operator~() const;
    UIntBatch operator&(const UIntBatch &rhs) const;
    UIntBatch operator|(const UIntBatch &rhs) const;
    UIntBatch operator^(const UIntBatch &rhs) const;
    UIntBatch operator&(uint64_t k) const;
    UIntBatch operator|(uint64_t k) const;
    UIntBatch operator^(uint64_t k) const;
    // public distance s; kept planes share the source's payload
    UIntBatch shiftLeft(unsigned s) const;
    UIntBatch shiftRight(unsigned s) const;
    UIntBatch rotateLeft(unsigned s) const;
    UIntBatch rotateRight(unsigned s) const;
    // ENCRYPTED distance d, element by element; d of the same context and count, any width
    UIntBatch shiftLeft(const UIntBatch &d) const;
    UIntBatch shiftRight(const UIntBatch &d) const;
    UIntBatch rotateLeft(const UIntBatch &d) const;
    UIntBatch rotateRight(const UIntBatch &d) const;
};

UIntBatch operator-(uint64_t k, const UIntBatch &a);

// Bit j of element e is Dec(bits[j][e]): 1 to 64 one-bit batches of one context and count (std::invalid_argument
// otherwise) packed into one word per element.  The batches need not be an integer's planes: a carry, a membership
// bit, the outputs of compareExchange pack the same way.  An empty batch gives an empty vector.
std::vector<uint64_t> decryptPacked(const std::vector<CiphertextBatch> &bits, const SecretKey &key);
// The route UIntBatch::decrypt takes for `a` under the calling thread's knobs (a static string): "call" (one
// csgn_uint_decrypt) or "planes" (one CiphertextBatch::decrypt per plane).  No device work; for diagnostics and tests,
// like arithRoute.
const char *decryptRoute(const UIntBatch &a);

// one encrypted bit per element
// The route a + b, a - b, equalTo, notEqualTo, lessThan and greaterThan take for operands of `width` planes, every one
// of them uniform or not, under the calling thread's knobs (a static string): "call" (csgn_uint_arith /
// csgn_uint_lt_select, in the form their own knobs choose) or "chain" (one step per bit).  No device work.  For
// diagnostics and for the tests that must show which route a forced knob gave (tests/test_uint_arith_cpp.py): the
// route is a speed matter, the words are the same, and a program should not branch on it.
const char *arithRoute(unsigned width, bool uniform_planes);
CiphertextBatch equalTo(const UIntBatch &a, const UIntBatch &b);
CiphertextBatch notEqualTo(const UIntBatch &a, const UIntBatch &b);
CiphertextBatch lessThan(const UIntBatch &a, const UIntBatch &b);
CiphertextBatch lessEqual(const UIntBatch &a, const UIntBatch &b);
CiphertextBatch greaterThan(const UIntBatch &a, const UIntBatch &b);
CiphertextBatch greaterEqual(const UIntBatch &a, const UIntBatch &b);
// against the public constant k (one encrypted bit per element)
CiphertextBatch equalTo(const UIntBatch &a, uint64_t k);
CiphertextBatch notEqualTo(const UIntBatch &a, uint64_t k);
CiphertextBatch lessThan(const UIntBatch &a, uint64_t k);
CiphertextBatch lessEqual(const UIntBatch &a, uint64_t k);
CiphertextBatch greaterThan(const UIntBatch &a, uint64_t k);
CiphertextBatch greaterEqual(const UIntBatch &a, uint64_t k);
// element i: sel[i] ? a[i] : b[i]
UIntBatch select(const CiphertextBatch &sel, const UIntBatch &a, const UIntBatch &b);
// element i: mask[i] ? a[i] : 0; plane j is mask * a_j.  mask of a's context and count
UIntBatch keepWhere(const CiphertextBatch &mask, const UIntBatch &a);
// The route a & b, a | b, a ^ b, ~a, select and keepWhere take (op: CSGN_UINT_BITWISE_* of csgn_hip.h) for a selector of
// sel_terms terms and planes of a_terms[j] / b_terms[j] terms (operands the op does not read: 0 / empty), every plane
// uniform or not (a static string): "call" (one csgn_uint_bitwise, in the form its knob chooses) or "planes" (the
// CiphertextBatch operators and Gates.h plane by plane; also for a shape the call would refuse).  No device work; for
// diagnostics and tests, like arithRoute: the words are the same.
const char *bitwiseRoute(int op, uint64_t sel_terms, const std::vector<uint64_t> &a_terms, const std::vector<uint64_t> &b_terms,
                         bool uniform_planes);

// element i: a[i] + (mask[i] ? k : 0) mod 2^width, k < 2^width public (the block "A PUBLIC CONSTANT WHERE AN ENCRYPTED
// FLAG IS SET" above); mask of a's context and count.  *carry_out (may be null) = the bit that left the top plane.
UIntBatch addWhere(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k, CiphertextBatch *carry_out = nullptr);
UIntBatch subWhere(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k);          // addWhere(mask, a, (2^w - k) mod 2^w)
UIntBatch incrementWhere(const CiphertextBatch &mask, const UIntBatch &a, CiphertextBatch *carry_out = nullptr);   // k = 1
UIntBatch decrementWhere(const CiphertextBatch &mask, const UIntBatch &a);                // k = 2^w - 1
// The route addWhere and its kin take for an integer of `width` planes, the mask and every plane uniform or not, under
// the calling thread's knobs (a static string): "call" (one csgn_uint_add_where) or "loop" (the table through the
// CiphertextBatch operators).  No device work; for diagnostics and tests, like arithRoute: the words are the same.
const char *addWhereRoute(unsigned width, bool uniform_operands);
// The same for one call's operands, with the per-shape rule of the measurement: the loop also for the shape class the
// one launch lost (one-term planes and mask, one set bit in k with 16 planes or more above it, 256 MiB of outputs or
// more), and for k = 0 and an empty batch, which launch nothing.
const char *addWhereRoute(const CiphertextBatch &mask, const UIntBatch &a, uint64_t k);

// A public matrix over F2 (the block "PUBLIC LINEAR MAPS OVER F2" above): outWidth() rows, row j the mask of the input
// bits (bit i: input bit i, below inWidth()) whose XOR is output bit j.  Host only, no device work.  Widths are 1..64;
// std::invalid_argument otherwise, for a row bit at or above the input width, and for operands of mismatched shapes.
class F2Matrix {
    std::vector<uint64_t> rows_;
    unsigned in_;
    F2Matrix(const std::vector<uint64_t> &rows, unsigned in_width) : rows_(rows), in_(in_width) {}

  public:
    static F2Matrix fromRows(const std::vector<uint64_t> &rows, unsigned in_width);
    static F2Matrix identity(unsigned w);
    static F2Matrix shiftLeft(unsigned w, unsigned s);      // x << s mod 2^w (s >= w: zero)
    static F2Matrix shiftRight(unsigned w, unsigned s);     // x >> s
    static F2Matrix rotateLeft(unsigned w, unsigned s);     // s taken mod w
    static F2Matrix rotateRight(unsigned w, unsigned s);
    static F2Matrix mask(unsigned w, uint64_t k);           // x & k, k < 2^w
    static F2Matrix clmul(unsigned w, uint64_t k);          // the carry-less product x * k mod 2^w, k < 2^w
    // x * k in GF(2^w) = F2[X] / poly, k < 2^w; poly holds the terms below X^w, and may hold X^w itself where it fits
    // (0x11B and 0x1B both name AES's field at w = 8)
    static F2Matrix gfMul(unsigned w, uint64_t k, uint64_t poly);
    static F2Matrix gfSquare(unsigned w, uint64_t poly);    // x * x in the same field: squaring is linear over F2
    static F2Matrix grayEncode(unsigned w);                 // x ^ (x >> 1)
    static F2Matrix grayDecode(unsigned w);                 // its inverse: bit j = the XOR of bits j .. w - 1

    unsigned inWidth() const { return in_; }
    unsigned outWidth() const { return (unsigned)rows_.size(); }
    const std::vector<uint64_t> &rows() const { return rows_; }
    uint64_t apply(uint64_t x) const;                       // the clear map: bit j = parity(rows[j] & x)
    F2Matrix operator^(const F2Matrix &rhs) const;          // x -> (*this)(x) ^ rhs(x); one shape
    // composition over F2: x -> (*this)(rhs(x)); inWidth() == rhs.outWidth().  Public duplicates cancel here.
    F2Matrix operator*(const F2Matrix &rhs) const;
    bool operator==(const F2Matrix &rhs) const { return in_ == rhs.in_ && rows_ == rhs.rows_; }
};

// element i: m(a[i]) ^ constant, of width m.outWidth(); a.width() == m.inWidth(), constant < 2^outWidth()
UIntBatch linearMap(const UIntBatch &a, const F2Matrix &m, uint64_t constant = 0);
// element i: the parity of a[i] & mask, one encrypted bit; mask < 2^width.  mask == 0 gives ZERO.
CiphertextBatch parity(const UIntBatch &a, uint64_t mask);
// The route linearMap takes (a static string): "call" (one csgn_uint_linear for every row that is neither a single
// input bit nor a constant) or "loop" (the CiphertextBatch operators row by row: a ragged plane; also when no row is
// left to compute or the batch is empty, which launch nothing).  No device work; for diagnostics and tests, like
// arithRoute: the words are the same.
const char *linearRoute(const UIntBatch &a, const F2Matrix &m, uint64_t constant = 0);

// A public bilinear form over F2 of two integers (the block "PUBLIC BILINEAR FORMS OVER F2" above): outWidth() rows, row
// j the list of the pairs (i, l) -- bit i of x below leftWidth(), bit l of y below rightWidth() -- whose products x_i y_l
// XOR to output bit j.  Host only, no device work.  A row is kept sorted by (left, right) with nothing twice: duplicates
// cancel over F2 here, where they are public.  Widths are 1..64; std::invalid_argument otherwise, for an index at or
// above its width, and for operands of mismatched shapes.
class F2Bilinear {
  public:
    typedef std::pair<unsigned, unsigned> Pair;             // (bit of x, bit of y)

  private:
    std::vector<std::vector<Pair> > rows_;
    unsigned left_, right_;
    F2Bilinear(const std::vector<std::vector<Pair> > &rows, unsigned left, unsigned right)
        : rows_(rows), left_(left), right_(right) {}

  public:
    // any order, repetitions allowed: a pair named an even number of times is gone
    static F2Bilinear fromPairs(const std::vector<std::vector<Pair> > &rows, unsigned left_width, unsigned right_width);
    static F2Bilinear clmul(unsigned w);                    // the carry-less product x * y mod 2^w: the low w planes
    static F2Bilinear clmulWide(unsigned w);                // all 2w - 1 planes of it, w <= 32
    // x * y in GF(2^w) = F2[X] / poly; poly as in F2Matrix::gfMul
    static F2Bilinear gfMul(unsigned w, uint64_t poly);
    static F2Bilinear bitwiseAnd(unsigned w);               // x & y
    static F2Bilinear dotBits(unsigned w);                  // parity(x & y): one plane

    unsigned leftWidth() const { return left_; }
    unsigned rightWidth() const { return right_; }
    unsigned outWidth() const { return (unsigned)rows_.size(); }
    const std::vector<std::vector<Pair> > &rows() const { return rows_; }
    uint64_t apply(uint64_t x, uint64_t y) const;           // the clear form
    F2Bilinear operator^(const F2Bilinear &rhs) const;      // (x, y) -> (*this)(x, y) ^ rhs(x, y); one shape
    // the form after linear maps of its arguments: (x, y) -> (*this)(on_a(x), on_b(y))
    F2Bilinear compose(const F2Matrix &on_a, const F2Matrix &on_b) const;
    bool operator==(const F2Bilinear &rhs) const { return left_ == rhs.left_ && right_ == rhs.right_ && rows_ == rhs.rows_; }
};
// the linear map after the form: (x, y) -> m(form(x, y)); m.inWidth() == form.outWidth().  gfMul(w, poly) IS the
// reduction matrix times clmulWide(w) for w <= 32.
F2Bilinear operator*(const F2Matrix &m, const F2Bilinear &form);

// element i: form(a[i], b[i]) ^ constant, of width form.outWidth(); a.width() == form.leftWidth(), b.width() ==
// form.rightWidth(), constant < 2^outWidth().  a and b may be the same integer.
UIntBatch bilinearMap(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &form, uint64_t constant = 0);
UIntBatch clmul(const UIntBatch &a, const UIntBatch &b);        // one width w; w planes
UIntBatch clmulWide(const UIntBatch &a, const UIntBatch &b);    // one width w <= 32; 2w - 1 planes
UIntBatch gfMul(const UIntBatch &a, const UIntBatch &b, uint64_t poly);
CiphertextBatch dotBits(const UIntBatch &a, const UIntBatch &b);   // parity(a[i] & b[i]), one encrypted bit
// The route bilinearMap takes (a static string): "k_uint_bilinear" (one csgn_uint_bilinear for all planes), "loop" (the
// CiphertextBatch operators plane by plane: a ragged plane) or "none" (an empty batch: nothing is launched).  No device work.
const char *bilinearRoute(const UIntBatch &a, const UIntBatch &b, const F2Bilinear &form, uint64_t constant = 0);

// element i: lo <= a[i] <= hi, one encrypted bit / its negation; lo <= hi < 2^width
CiphertextBatch inRange(const UIntBatch &a, uint64_t lo, uint64_t hi);
CiphertextBatch outOfRange(const UIntBatch &a, uint64_t lo, uint64_t hi);
// element i: a[i] lies in one of the disjoint ascending intervals (lo, hi)
CiphertextBatch inRanges(const UIntBatch &a, const std::vector<std::pair<uint64_t, uint64_t> > &intervals);
// element i: a[i] is / is not a value of the set (any order, duplicates allowed); an empty set gives ZERO / ONE
CiphertextBatch isIn(const UIntBatch &a, const std::vector<uint64_t> &set);
CiphertextBatch notIn(const UIntBatch &a, const std::vector<uint64_t> &set);
// element i: values[number of thresholds <= a[i]], of out_width bits; thresholds strictly ascending in 1 .. 2^width - 1
UIntBatch stepFunction(const UIntBatch &a, const std::vector<uint64_t> &thresholds, const std::vector<uint64_t> &values,
                       unsigned out_width);
// element i: the number of thresholds <= a[i], of `planes` bits (thresholds.size() < 2^planes)
UIntBatch bucketOf(const UIntBatch &a, const std::vector<uint64_t> &thresholds, unsigned planes);
// element i: values[r] where a[i] == keys[r], else `otherwise`, of out_width bits
UIntBatch lookupSparse(const UIntBatch &a, const std::vector<uint64_t> &keys, const std::vector<uint64_t> &values,
                       unsigned out_width, uint64_t otherwise = 0);
// The route stepFunction(a, thresholds, values, out_width) takes (a static string): "call" (one csgn_uint_plain_sum for
// every plane that is neither a constant nor a single comparison) or "loop" (the comparisons and operator+ plane by
// plane: a ragged plane; also when no plane is left to compute or the batch is empty).  No device work.
const char *plainSumRoute(const UIntBatch &a, const std::vector<uint64_t> &thresholds, const std::vector<uint64_t> &values,
                          unsigned out_width);

// element i: a[i] < b[i] ? a[i] : b[i] / the other one; a tie takes b for min and a for max
UIntBatch min(const UIntBatch &a, const UIntBatch &b);
UIntBatch max(const UIntBatch &a, const UIntBatch &b);
// (min, max) from one launch
std::pair<UIntBatch, UIntBatch> minMax(const UIntBatch &a, const UIntBatch &b);
// element i: a[i] < b[i] ? x[i] : y[i]; x and y of one width (any), a and b of one width
UIntBatch selectLess(const UIntBatch &a, const UIntBatch &b, const UIntBatch &x, const UIntBatch &y);
CiphertextBatch selectLess(const UIntBatch &a, const UIntBatch &b, const CiphertextBatch &x, const CiphertextBatch &y);
// *lo = min, *hi = max, *plo = a < b ? pa : pb, *phi = a < b ? pb : pa, all from the same launch; null outputs are
// skipped.  A tie: lo = b, hi = a, plo = pb, phi = pa.  pa and pb of one width (any).
void compareExchange(const UIntBatch &a, const UIntBatch &b, const UIntBatch &pa, const UIntBatch &pb, UIntBatch *lo,
                     UIntBatch *hi, UIntBatch *plo, UIntBatch *phi);

// A public table compiled once; copies share the compiled form.  Safe to use from several threads at once.
class LookupTable {
  public:
    struct Impl;
    // table.size() == 2^in_width, every entry < 2^out_width (std::invalid_argument otherwise)
    LookupTable(const std::vector<uint64_t> &table, unsigned in_width, unsigned out_width);
    unsigned inWidth() const;
    unsigned outWidth() const;
    const std::vector<uint64_t> &table() const;
    const std::vector<uint64_t> &anf() const;      // bit j of anf()[S]: monomial S of output j
    const std::shared_ptr<Impl> &impl() const { return impl_; }

  private:
    std::shared_ptr<Impl> impl_;
};

// A public polynomial over F2 of several integers (the block "PUBLIC POLYNOMIAL MAPS OVER F2" above).  The operands
// have the widths widths() (each 1..64, 256 bits in all); bit i of operand o is the VARIABLE (the sum of the widths
// before o) + i.  outWidth() rows (1..64); row j is a set of monomials, a monomial a set of variables whose product
// XORs into output bit j, plus the row's bit of constant().  Host only, no device work.  A row is kept canonical: the
// variables of a monomial ascending with none twice (x x = x), the monomials ascending by (degree, then the variables),
// none twice (duplicates cancel over F2 here, where they are public), a monomial of no variable folded into the
// constant.  std::invalid_argument for widths outside these limits, a variable at or above variables(), a degree above
// 8, operands of mismatched shapes, and a result past 262144 monomials.
class F2Polynomial {
  public:
    typedef std::vector<unsigned> Monomial;                 // variables
    typedef std::vector<std::vector<Monomial> > Rows;

  private:
    Rows rows_;
    std::vector<unsigned> widths_;
    uint64_t constant_;
    F2Polynomial(const Rows &rows, const std::vector<unsigned> &widths, uint64_t constant)
        : rows_(rows), widths_(widths), constant_(constant) {}

  public:
    // any order, repetitions allowed: a monomial named an even number of times is gone; an empty monomial is the constant
    static F2Polynomial fromMonomials(const Rows &rows, const std::vector<unsigned> &widths);
    static F2Polynomial linear(const F2Matrix &m);          // one operand; linearMap's words
    static F2Polynomial bilinear(const F2Bilinear &f);      // two operands; bilinearMap's words
    static F2Polynomial fromLookupTable(const LookupTable &f);   // one operand; the table's ANF, of degree <= 8
    static F2Polynomial ch(unsigned w);                     // (e, f, g) -> (e & f) ^ (~e & g) = ef + eg + g
    static F2Polynomial maj(unsigned w);                    // (a, b, c) -> ab + ac + bc
    static F2Polynomial chi(unsigned w);                    // (x, y, z) -> x ^ (~y & z) = x + z + yz
    static F2Polynomial andAll(unsigned w, unsigned k);     // the AND of k operands of w bits, 1 <= k <= 8
    static F2Polynomial mux(unsigned w);                    // (s, x, y) -> s ? x : y, s of one bit

    const std::vector<unsigned> &widths() const { return widths_; }
    unsigned variables() const;                             // the sum of the widths
    unsigned outWidth() const { return (unsigned)rows_.size(); }
    const Rows &rows() const { return rows_; }
    uint64_t constant() const { return constant_; }
    uint64_t apply(const std::vector<uint64_t> &operands) const;   // the clear value, the constant included
    F2Polynomial operator^(const F2Polynomial &rhs) const;  // one shape
    // the pointwise product, bit j = (*this)_j & rhs_j: monomials multiply, variables merge, duplicates cancel
    F2Polynomial operator&(const F2Polynomial &rhs) const;
    // the form after a linear map of each operand: on[o].outWidth() == widths()[o]; the new widths are on[o].inWidth()
    F2Polynomial compose(const std::vector<F2Matrix> &on) const;
    bool operator==(const F2Polynomial &rhs) const
    {
        return widths_ == rhs.widths_ && rows_ == rhs.rows_ && constant_ == rhs.constant_;
    }
};
// the linear map after the form: m.inWidth() == form.outWidth()
F2Polynomial operator*(const F2Matrix &m, const F2Polynomial &form);

// element i: f(operands[0][i], operands[1][i], ...) ^ constant, of width f.outWidth(); the operands' widths are
// f.widths(), constant < 2^outWidth().  Operands may be the same integer.
UIntBatch polyMap(const std::vector<UIntBatch> &operands, const F2Polynomial &f, uint64_t constant = 0);
UIntBatch ch(const UIntBatch &e, const UIntBatch &f, const UIntBatch &g);     // one width
UIntBatch maj(const UIntBatch &a, const UIntBatch &b, const UIntBatch &c);
UIntBatch chi(const UIntBatch &a, const UIntBatch &b, const UIntBatch &c);    // a ^ (~b & c)
UIntBatch andAll(const std::vector<UIntBatch> &operands);                     // 1 to 8 operands of one width
// The route polyMap takes (a static string): "k_uint_poly" (one csgn_uint_poly for every row that is neither a single
// input bit nor a constant), "loop" (the CiphertextBatch operators: a ragged plane) or "none" (an empty batch, or no row
// left to compute: nothing is launched).  No class of shapes is routed elsewhere.  No device work.
const char *polyRoute(const std::vector<UIntBatch> &operands, const F2Polynomial &f, uint64_t constant = 0);

// f(a), a.width() == f.inWidth(); f.outWidth() planes
UIntBatch lookup(const UIntBatch &a, const LookupTable &f);
// f(a + (b << a.width())), a.width() + b.width() == f.inWidth(); one context and element count
UIntBatch lookup(const UIntBatch &a, const UIntBatch &b, const LookupTable &f);

// element e: table[index[e]] where index[e] < table.size(), else 0; one output plane per table plane
UIntBatch readAt(const UIntBatch &table, const UIntBatch &index);
CiphertextBatch readAt(const CiphertextBatch &table, const UIntBatch &index);

// element e: arrays[e * n + index[e]] where index[e] < n, else 0; arrays.size() == n * index.size(), 1 <= n <= 2^v
UIntBatch readAtEach(const UIntBatch &arrays, uint64_t n, const UIntBatch &index);
CiphertextBatch readAtEach(const CiphertextBatch &arrays, uint64_t n, const UIntBatch &index);
// The route readAtEach takes for these operands (a static string): "pick" (uniform planes of one term count under a
// uniform index of at most 16 bits: one csgn_uint_pick), "rows" (planes whose terms have period n under such an index --
// writeAtEach's results: one csgn_uint_pick_rows) or "loop" (anything else, a compact()ed index for one: equalTo, gather,
// operator* and operator+ row by row).  No device work; for diagnostics and tests, like arithRoute and decryptRoute: the
// words are the same on every route.
const char *readAtEachRoute(const UIntBatch &arrays, uint64_t n, const UIntBatch &index);

// the arrays with element e * n + index[e] replaced by value[e] where index[e] < n; arrays.size() == n * index.size(),
// 1 <= n <= 2^v, value of the arrays' width and the index's count.  The result's planes are ragged (see above)
UIntBatch writeAtEach(const UIntBatch &arrays, uint64_t n, const UIntBatch &index, const UIntBatch &value);
CiphertextBatch writeAtEach(const CiphertextBatch &arrays, uint64_t n, const UIntBatch &index,
                            const CiphertextBatch &value);
// ONE index and value: the table with row index[0] replaced; writeAtEach with n = table.size()
UIntBatch writeAt(const UIntBatch &table, const UIntBatch &index, const UIntBatch &value);

// element e: XOR over rows r with keys[r] == query[e] of values[r]  (distinct keys: the matching value, else 0)
UIntBatch readWhere(const UIntBatch &keys, const UIntBatch &values, const UIntBatch &query);
CiphertextBatch readWhere(const UIntBatch &keys, const CiphertextBatch &values, const UIntBatch &query);
// the same, and *member = matches(keys, query) from the same launch (member may be null)
UIntBatch readWhere(const UIntBatch &keys, const UIntBatch &values, const UIntBatch &query, CiphertextBatch *member);
// element e: parity of the number of rows with keys[r] == query[e]  (distinct keys: membership)
CiphertextBatch matches(const UIntBatch &keys, const UIntBatch &query);

// element q: the number of ones among bits[q*group .. q*group+group-1], modulo 2^planes; planes >= 1
UIntBatch countOnes(const CiphertextBatch &bits, uint64_t group, unsigned planes);
// bit j alone of that number (j = 6 at group 64: the AND of all 64); ZERO where 2^j > group
CiphertextBatch countBit(const CiphertextBatch &bits, uint64_t group, unsigned j);
// Hamming weight of every element, modulo 2^planes / its bit j alone
UIntBatch popcount(const UIntBatch &a, unsigned planes);
CiphertextBatch popcountBit(const UIntBatch &a, unsigned j);
// popcount(a ^ b, planes)
UIntBatch hammingDistance(const UIntBatch &a, const UIntBatch &b, unsigned planes);
// element e: the number of rows r with keys[r] == query[e], modulo 2^planes: countOnes over the batch whose element
// e*n + r is equalTo(keys row r, query element e); plane 0 has the words of matches(keys, query)
UIntBatch countMatches(const UIntBatch &keys, const UIntBatch &query, unsigned planes);

// entry r, 0 <= r < group: element q is the number of ones among bits[q*group .. q*group+r] -- with `exclusive` among
// the r bits before row r --, modulo 2^planes: word for word countOnes of those rows, ZERO planes included
std::vector<UIntBatch> runningCount(const CiphertextBatch &bits, uint64_t group, unsigned planes, bool exclusive = false);
// bit j alone of every entry (j = 0: the running parity)
std::vector<CiphertextBatch> runningCountBit(const CiphertextBatch &bits, uint64_t group, unsigned j, bool exclusive = false);
// of an integer's own planes (the plane layout): entry i is the number of set bits among bits 0..i of a -- below bit i
// with `exclusive`: the rank function of a bit vector --, modulo 2^planes
std::vector<UIntBatch> prefixPopcount(const UIntBatch &a, unsigned planes, bool exclusive = false);
// The route the three functions above take for groups of `group` rows (an integer's planes: its width), every input
// uniform with one term count, or not (a static string): "csgn_count_prefix" (one call, one launch) or "loop" (the
// gathered prefix through countOnes' route row by row).  No device work, like nthRoute: the words are the same.
const char *runningCountRoute(uint64_t group, bool uniform_operands);

// element q: the sum of a[q*group .. q*group+group-1], modulo 2^planes; planes >= 1 / its bit j alone
UIntBatch sumValues(const UIntBatch &a, uint64_t group, unsigned planes);
CiphertextBatch sumBit(const UIntBatch &a, uint64_t group, unsigned j);
// element q: the sum over the group's rows r of mask[r] ? values[r] : 0, modulo 2^planes: SUM(value) WHERE mask
UIntBatch sumWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, unsigned planes);
// element i: a[i] * b[i] modulo 2^planes; one context and element count, any widths
UIntBatch mul(const UIntBatch &a, const UIntBatch &b, unsigned planes);
// element q: the sum over the group's rows r of a[r] * b[r], modulo 2^planes
UIntBatch innerProduct(const UIntBatch &a, const UIntBatch &b, uint64_t group, unsigned planes);


// element q: values[q*group + r] for the first r with mask[q*group + r] set, 0 when none; *any (may be null): the OR
UIntBatch firstWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, CiphertextBatch *any = nullptr);
CiphertextBatch firstWhere(const CiphertextBatch &mask, const CiphertextBatch &values, uint64_t group,
                           CiphertextBatch *any = nullptr);
// element q: the OR of bits[q*group .. q*group+group-1]
CiphertextBatch anyOf(const CiphertextBatch &bits, uint64_t group);
// element q: the r of the first set mask[q*group + r], modulo 2^planes (0 when none; *any tells)
UIntBatch firstIndex(const CiphertextBatch &mask, uint64_t group, unsigned planes, CiphertextBatch *any = nullptr);
// of an integer's own planes (the plane layout): the index of the lowest set bit modulo 2^planes (0 where a == 0;
// *nonzero tells), a & -a, and the bit length modulo 2^planes (labels width - r over the planes taken from the top; 0
// where a == 0)
UIntBatch lowestSetIndex(const UIntBatch &a, unsigned planes, CiphertextBatch *nonzero = nullptr);
UIntBatch lowestSetBit(const UIntBatch &a);
UIntBatch bitLength(const UIntBatch &a, unsigned planes);
// The route the seven functions above take for groups of `group` rows (an integer's planes: its width), every operand
// uniform -- and, in the grouped layout, the mask of one term count -- or not (a static string): "call" (one
// csgn_uint_first) or "loop" (gather, logicNot, operator* and operator+ row by row; also for a group the call would
// refuse).  No device work; for diagnostics and tests, like arithRoute: the words are the same.
const char *firstRoute(uint64_t group, bool uniform_operands);

// element q: values[q*group + r] for the (slot + 1)-th r with mask[q*group + r] set, 0 when at most `slot` are; *valid
// (may be null): more than `slot` are set
UIntBatch nthWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, uint64_t slot,
                   CiphertextBatch *valid = nullptr);
CiphertextBatch nthWhere(const CiphertextBatch &mask, const CiphertextBatch &values, uint64_t group, uint64_t slot,
                         CiphertextBatch *valid = nullptr);
// slots 0 .. k-1 (k in 1..group; one call a slot): the matching rows compacted to the front, in order; (*valid)[s]
std::vector<UIntBatch> takeWhere(const CiphertextBatch &mask, const UIntBatch &values, uint64_t group, uint64_t k,
                                 std::vector<CiphertextBatch> *valid = nullptr);
// element q: the r of the (slot + 1)-th set mask[q*group + r], modulo 2^planes (0 when there is none; *valid tells)
UIntBatch nthIndex(const CiphertextBatch &mask, uint64_t group, uint64_t slot, unsigned planes,
                   CiphertextBatch *valid = nullptr);
// of an integer's own planes (the plane layout): the position of the (slot + 1)-th set bit, modulo 2^planes
UIntBatch nthSetIndex(const UIntBatch &a, uint64_t slot, unsigned planes, CiphertextBatch *valid = nullptr);
// element q: at least k of bits[q*group .. q*group+group-1] are set (*valid of slot k - 1; k == 0: ONE; k > group: ZERO)
CiphertextBatch atLeast(const CiphertextBatch &bits, uint64_t group, uint64_t k);
// at least k of a's bits are set (the plane layout); hammingDistance(a, b) <= r is logicNot(popcountAtLeast(a ^ b, r + 1))
CiphertextBatch popcountAtLeast(const UIntBatch &a, uint64_t k);
// The route the seven functions above take for groups of `group` rows (an integer's planes: its width), every operand
// uniform and the mask rows of one term count, or not (a static string): "call" (one csgn_uint_nth a slot) or "loop"
// (gather, operator* and operator+ subset by subset; also for a group the call would refuse).  No device work; for
// diagnostics and tests, like firstRoute: the words are the same.
const char *nthRoute(uint64_t group, bool uniform_operands);

} // namespace certFHE

#endif
