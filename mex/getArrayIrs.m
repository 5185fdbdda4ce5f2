function irs = getArrayIrs(sources, fs, irLen, preDelay, micRadius, micGridAziZenRad, varargin)
% Impulse responses of the simulated rigid-sphere array (the array of getSMAIRMatrix) to sources that are sums of plane-wave
% components, on the MI355X library (DESIGN.md section 11; include/emagls.h, emagls_array_irs): per source, microphone and bin
%   H(k, m) = sum_j g_j exp(-2 pi i k (tau_j + preDelay) / nfft) * pwGrid_k(m, dir_j),
% pwGrid_k the operand of getEMagLs2Filters, then irfft at length nfft and the first irLen samples.
%   irs = getArrayIrs(sources, fs, irLen, preDelay, micRadius, micGridAziZenRad, 'name', value, ...)
%   sources   [Q x 2] directions (azimuth, zenith), one unit plane wave each: a direction bank for a moving virtual source; or a
%             cell of Q arrays [J_q x 2|3|4] with the columns azimuth, zenith, delay in samples (default 0), gain (default 1): an
%             array room response from the image sources the caller lists (a source may be empty)
%   preDelay  samples (fractional allowed): makes the acausal part of the sphere's response causal
%   further names: order (4; only enters the simulation order max(order, ceil(fs*pi*micRadius/343))), encoder ([]: raw microphones;
%             [numChannels x numMics], real or complex, e.g. pinv(getSH(order, micGridAziZenRad, shDefinition))), nfft ([]: the
%             smallest power of two >= 2*irLen)
%   the spectral gain (DESIGN.md section 13; emagls_array_irs_spectral), all [] by default: surfaceReflection [W x P], W <= 8 real
%             reflection spectra in [-1, 1] over the P = nfft/2 + 1 bins, with exponents, a cell like sources of integer arrays
%             [J_q x W]; airAttenuation [P] in Np/m with pathLength, a cell of [J_q x 1] arrays in metres (both or neither).  The gain
%             of a component becomes gain * prod_w R_w(k)^e_w * exp(-alpha(k) * l) in bin k
%   point sources (DESIGN.md section 14; emagls_array_irs_point): distance ([]), a cell like sources of [J_q x 1] arrays in metres (or
%             [Q x 1] for the [Q x 2] form), every value finite and greater than micRadius, for all components or for none.  The
%             order-n term of a component then carries the near-field factor F_n(kappa*rho); delay and gain stay the caller's
%   directive sources (DESIGN.md section 15; emagls_array_irs_directive): directivity ([]), [Q x Kd x P] real or complex coefficients of
%             each source's directivity per bin in the real basis of getSH(Nd, ., 'real'), Kd = (Nd + 1)^2, Nd <= 8 ([Q x Kd] or a vector
%             [Kd] is repeated over bins and sources; firstOrderDirectivity makes first-order patterns); emission, a cell like sources of
%             [J_q x 3] unit vectors in room axes along which each component's ray left the real source ([Q x 3] for the [Q x 2] form;
%             the further output of getShoeboxComponents / getShoeboxImages); sourceOrientation ([]: the room's axes), [3 x 3 x Q]
%             rotation matrices whose columns are each source's front, left and up axes, or [Q x 2] = (azimuth, zenith) of the front axis
%   irs       [irLen x numChannels x Q] (complex with a complex encoder): irs(:, :, q) is the rir of sourceFieldStream
p = struct('order', 4, 'encoder', [], 'nfft', [], 'surfaceReflection', [], 'exponents', [], 'airAttenuation', [], 'pathLength', [], 'distance', [], ...
    'emission', [], 'sourceOrientation', [], 'directivity', []);
for i = 1:2:numel(varargin)
    if ~isfield(p, varargin{i}); error('eMagLS:arg', 'unknown option "%s"', varargin{i}); end
    p.(varargin{i}) = varargin{i + 1};
end
if ~iscell(sources)
    if size(sources, 2) ~= 2; error('eMagLS:arg', 'sources must be [Q x 2] directions or a cell of [J x 2|3|4] arrays'); end
    sources = num2cell(double(sources), 2);
end
Q = numel(sources);
compPtr = zeros(Q + 1, 1);
comps = zeros(0, 4);
for q = 1:Q
    s = double(sources{q});
    if isempty(s); s = zeros(0, 2); end
    if ~any(size(s, 2) == [2 3 4]); error('eMagLS:arg', 'every source must be [J x 2|3|4] (azimuth, zenith, delay, gain)'); end
    J = size(s, 1);
    if size(s, 2) < 3; s(:, 3) = zeros(J, 1); end
    if size(s, 2) < 4; s(:, 4) = ones(J, 1); end
    comps = [comps; s]; %#ok<AGROW>
    compPtr(q + 1) = compPtr(q) + J;
end
exps = [];
paths = [];
if ~isempty(p.surfaceReflection) || ~isempty(p.airAttenuation)
    if ~isempty(p.surfaceReflection); exps = zeros(0, size(p.surfaceReflection, 1)); end
    for q = 1:Q
        if ~isempty(p.surfaceReflection); exps = [exps; reshape(double(p.exponents{q}), [], size(exps, 2))]; end %#ok<AGROW>
        if ~isempty(p.airAttenuation); paths = [paths; reshape(double(p.pathLength{q}), [], 1)]; end %#ok<AGROW>
    end
    if ~isempty(p.airAttenuation) && isempty(paths); paths = 0; end
end
dists = [];
if ~isempty(p.distance)
    if ~iscell(p.distance); p.distance = num2cell(double(p.distance(:))); end
    if numel(p.distance) ~= Q; error('eMagLS:arg', 'distance must hold one array per source'); end
    for q = 1:Q
        dists = [dists; reshape(double(p.distance{q}), [], 1)]; %#ok<AGROW>
    end
    if numel(dists) ~= size(comps, 1); error('eMagLS:arg', 'distances are given for all components of a call or for none'); end
end
emit = [];
rot = [];
coef = [];
if isempty(p.directivity) && (~isempty(p.emission) || ~isempty(p.sourceOrientation))
    error('eMagLS:arg', 'emission and sourceOrientation come with a directivity');
end
if ~isempty(p.directivity)
    if ~iscell(p.emission); p.emission = num2cell(double(p.emission), 2); end
    if numel(p.emission) ~= Q; error('eMagLS:arg', 'emission must hold one array per source'); end
    emit = zeros(0, 3);
    for q = 1:Q
        emit = [emit; reshape(double(p.emission{q}), [], 3)]; %#ok<AGROW>
    end
    nfft = double(p.nfft);
    if isempty(nfft); nfft = min(65536, max(8, 2^nextpow2(2 * double(irLen)))); end
    [rot, coef] = emaglsDirectiveArgs(p.sourceOrientation, p.directivity, Q, nfft / 2 + 1);
end
irs = emagls_mex('array_irs', compPtr, comps, double(fs), double(irLen), double(preDelay), double(micRadius), double(micGridAziZenRad), ...
    double(p.order), double(p.encoder), double(p.nfft), double(p.surfaceReflection), exps, double(p.airAttenuation(:)), paths, dists, emit, rot, coef);
end
