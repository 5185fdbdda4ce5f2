function [H, metrics] = getRenderedHrtfs(wL, wR, model, dirsAziZenRad, fs, varargin)
% What a set of decoding filters renders for a plane wave from each evaluation direction, on the MI355X library (DESIGN.md
% section 10; include/emagls.h, emagls_rendered_hrtfs):  Hhat_e(k, d) = sum_c fft(w_e, nfft)(k, c) * pwGrid_k(c, d), with pwGrid_k the
% operand of the matching design (lib/getEMagLsFilters.m:51-68, :87-103).
%   [H, metrics] = getRenderedHrtfs(wL, wR, model, dirsAziZenRad, fs, 'name', value, ...)
%   wL, wR   [len x numChannels] or [len x numChannels x numSets]
%   model    'sh' (order) | 'emagls' (order, micRadius, micGridAziZenRad) | 'emagls2' (micRadius, micGridAziZenRad) |
%            'atf' (atfIrs [taps x numMics x numDirections], given ON the evaluation directions) |
%            'ema_ch' | 'ema_sh' (order, micRadius, micGridAziZenRad): an equatorial array as getEMagLsFiltersEMAinCH (2*order+1
%            circular-harmonic channels, order <= 15) and getEMagLsFiltersEMAinSH ((order+1)^2 channels, order <= 7) model it;
%            micGridAziZenRad is then a vector of azimuths, or [numMics x 2] with every zenith pi/2
%   further names: nfft (default min(2048, 2*len)), shDefinition ('real'), hL, hR ([numSamples x numDirections (x numSets)]),
%   weights ([numDirections], uniform if absent), returnResponse (true)
%   H        [nfft/2+1 x numDirections x 2 x numSets] ([] with returnResponse false)
%   metrics  struct (empty fields without hL, hR): magErrDb [P x 2 x numSets], ildErrDb [P x numSets], covHat, covRef
%            [P x 4 x numSets] = (R_LL, R_RR, Re R_LR, Im R_LR), coherenceHat, coherenceRef [P x numSets]
p = struct('order', [], 'micRadius', [], 'micGridAziZenRad', [], 'atfIrs', [], 'nfft', [], 'shDefinition', 'real', 'hL', [], 'hR', [], ...
           'weights', [], 'returnResponse', true);
for i = 1:2:numel(varargin)
    if ~isfield(p, varargin{i}); error('eMagLS:arg', 'unknown option "%s"', varargin{i}); end
    p.(varargin{i}) = varargin{i + 1};
end
if isreal(wL) ~= isreal(wR); wL = complex(wL); wR = complex(wR); end
[H, m.magErrDb, m.ildErrDb, m.covHat, m.covRef] = emagls_mex('rendered_hrtfs', double(wL), double(wR), model, double(dirsAziZenRad), ...
    double(fs), double(p.order), double(p.micRadius), double(p.micGridAziZenRad), double(p.atfIrs), double(p.nfft), p.shDefinition, ...
    double(p.hL), double(p.hR), double(p.weights), logical(p.returnResponse));
coh = @(c) squeeze(hypot(c(:, 3, :), c(:, 4, :)) ./ sqrt(c(:, 1, :) .* c(:, 2, :)));
if ~isempty(m.covHat); m.coherenceHat = coh(m.covHat); m.coherenceRef = coh(m.covRef); else; m.coherenceHat = []; m.coherenceRef = []; end
metrics = m;
end
